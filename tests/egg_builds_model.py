"""numpy restatement of the three builds of src/app_egg.h: SBX_APP_EGG ("default", as shipped: `#define BEZIER` at :37 and the
`#if 1` egg of :46-52), SBX_APP_EGG_STRAIGHT ("straight", the BEZIER line removed: the four sd_cylinder legs of :86-109) and
SBX_APP_EGG_OVAL ("oval", the `#if 1` at :46 turned to `#if 0`: the one scaled sphere of :53-66); include/sbx.h, DESIGN.md §5.12.

The CPU oracle renders the shipped build only and is not to grow, so the GPU tests of the two other builds compare against this
module.  It is pinned from two sides (tests/test_egg_builds_cpu.py): build "default" equals Oracle.render("egg") in every bit —
which covers everything the three builds share: camera, turntable, pedals, IK, feet, wheel, ground, the unions, trace, shadow
march, colours, depth, bars, epilogue — and builds "straight" / "oval" equal frames and points that the reference header itself
rendered with the one line edited (tests/golden/egg_builds/, tools/make_golden_builds.py).

mainImage -> render -> render_scene -> sdf / shadowmarch, vectorised over pixels, in binary32 step by step in the oracle's
operation order (oracle/ovec.h: dot = (x x + y y) + z z, normalize = three divisions by sqrtf, M * v = (c0 v.x + c1 v.y) + c2 v.z
with its zero terms; oracle/sbx_math_ref.h: min / max as compare-and-select, mix = x (1 - a) + y a), every value an explicit
np.float32 so that nothing widens to float64.  sin, cos and pow are the oracle's (Oracle.math).  What sdf() computes from u_time
alone (src/app_egg.h:40, 68-96, 120, 125) is evaluated once per frame (`scene`), in the same operations; sdf is pinned against the
oracle's hook `egg.sdf`.  The vector algebra and the camera are tests/model_common.py's.
"""
import concurrent.futures
import functools

import numpy as np

from tests.model_common import (F, ONE, TWO, ZERO, _const, _f, _sincos, builds_fixture, cross, dot, fmax, fmin, get_primary_ray,
                                 normalize, op_add2, oracle, point_cam, same_bits)

HALF = F(.5)
BUILDS = ("default", "straight", "oval")
APP_OF = {"default": "egg", "straight": "egg_straight", "oval": "egg_oval"}
EYE, LOOK_AT = (F(.0), F(.25), F(5.25)), (F(.0), F(.25), F(.0))      # :23-27
MAT_EGG, MAT_BIKE, MAT_GROUND = 1, 2, 3             # :17-20
COLORS = {MAT_GROUND: (F(13.) / F(255.), F(104.) / F(255.), F(0.) / F(255.)), MAT_EGG: (F(0.9), F(0.95), F(0.95)),
          MAT_BIKE: (F(.2), F(.2), F(.2))}          # illuminate :29-35
THICK = F(.05)
FOV = F(1.)                                         # :253


def mat_vec(m, v):
    """M * v for columns m = (c0, c1, c2): (c0 v.x + c1 v.y) + c2 v.z (oracle/ovec.h:92), zero terms included"""
    return tuple((m[0][k] * v[0] + m[1][k] * v[1]) + m[2][k] * v[2] for k in range(3))


def rotate_around_y(deg):                           # util.h:53-60
    s, c = _sincos(deg)
    return ((c, ZERO, s), (ZERO, ONE, ZERO), (-s, ZERO, c))


def rotate_around_z(deg):                           # util.h:44-51
    s, c = _sincos(deg)
    return ((c, -s, ZERO), (s, c, ZERO), (ZERO, ZERO, ONE))


def length3(v):
    return np.sqrt(dot(v, v))


def sub3(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def add3(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def neg3(a):
    return (-a[0], -a[1], -a[2])


def clamp(x, lo, hi):                               # m_clamp
    return fmin(fmax(x, lo), hi)


def mix(x, y, a):                                   # m_mix
    return x * (ONE - a) + y * a


def op_blend(a, b, k):                              # sdf.h:38-47
    h = clamp(HALF + HALF * (b - a) / k, ZERO, ONE)
    return mix(b, a, h) - k * h * (ONE - h)


def ik_solver(start, goal_abs, l1, l2):             # IK.h:5-52
    goal = sub3(goal_abs, start)
    g = length3(goal)
    cos_theta = (l1 * l1 + g * g - l2 * l2) / (TWO * l1 * g)
    sin_theta = np.sqrt(ONE - cos_theta * cos_theta)
    rot = ((cos_theta, -sin_theta, ZERO), (sin_theta, cos_theta, ZERO), (ZERO, ZERO, ONE))
    n = normalize(goal)
    return add3(start, mat_vec(rot, (n[0] * l1, n[1] * l1, n[2] * l1)))


def sd_cylinder(P, P1, R):                          # sdf.h:95-109 with P0 = (0, 0, 0)
    P0 = (ZERO, ZERO, ZERO)
    d = normalize(sub3(P1, P0))
    dist = length3(cross(d, sub3(P, P0)))
    plane_1 = dot(d, P) + length3(P1)
    plane_2 = dot(neg3(d), P) + (-length3(P0))
    return fmax(fmax(dist, -plane_1), -plane_2) - R  # op_sub(op_sub(dist, plane_1), plane_2) - R


def det2(a, b):                                     # sdf.h:114-119
    return a[0] * b[1] - b[0] * a[1]


def sd_bezier_x(a, b, c, p, thickness):             # sdf.h:120-159, .x
    w = normalize(cross(sub3(c, b), sub3(a, b)))
    u = normalize(sub3(c, b))
    v = normalize(cross(w, u))
    ab, cb, pb = sub3(a, b), sub3(c, b), sub3(p, b)
    a2 = (dot(ab, u), dot(ab, v))
    c2 = (dot(cb, u), dot(cb, v))
    p3 = (dot(pb, u), dot(pb, v), dot(pb, w))
    b0 = (a2[0] - p3[0], a2[1] - p3[1])
    b1 = (ZERO - p3[0], ZERO - p3[1])
    b2 = (c2[0] - p3[0], c2[1] - p3[1])
    A = det2(b0, b2)
    B = TWO * det2(b1, b0)
    D = TWO * det2(b2, b1)
    f = B * D - A * A
    d21 = (b2[0] - b1[0], b2[1] - b1[1])
    d10 = (b1[0] - b0[0], b1[1] - b0[1])
    d20 = (b2[0] - b0[0], b2[1] - b0[1])
    gf = tuple(TWO * ((B * d21[k] + D * d10[k]) + A * d20[k]) for k in range(2))
    gf = (gf[1], -gf[0])
    den = gf[0] * gf[0] + gf[1] * gf[1]
    pp = ((-f) * gf[0] / den, (-f) * gf[1] / den)
    d0p = (b0[0] - pp[0], b0[1] - pp[1])
    ap = det2(d0p, d20)
    bp = TWO * det2(d10, d0p)
    t = clamp((ap + bp) / ((TWO * A + B) + D), ZERO, ONE)
    q = tuple(mix(mix(b0[k], b1[k], t), mix(b1[k], b2[k], t), t) for k in range(2))
    return F(0.85) * (np.sqrt((q[0] * q[0] + q[1] * q[1]) + p3[2] * p3[2]) - thickness)


# ---- the scene -----------------------------------------------------------------------------------------------------------

_SCENES = {}


def scene(u_time):
    """what sdf() (:38-144) computes from u_time alone, in its operations"""
    key = np.asarray(u_time, dtype=F).tobytes()
    if key not in _SCENES:
        with np.errstate(all="ignore"):
            t = F(u_time)
            S = {"rot_y": rotate_around_y(t * F(-100.0))}                                # :40
            wheel_pos = (ZERO, F(1.2), ZERO)
            pedal_radius, pedal_speed, pedal_off = F(0.3), F(400.), F(0.2)
            rot_z = rotate_around_z(-t * pedal_speed)                                    # :73, :76
            S["left_foot"] = add3(wheel_pos, mat_vec(rot_z, (ZERO, pedal_radius, pedal_off)))
            S["right_foot"] = add3(wheel_pos, mat_vec(rot_z, (ZERO, -pedal_radius, -pedal_off)))
            side = (ZERO, ZERO, pedal_off)
            femur, tibia = F(0.8), F(0.75)
            zero = (ZERO, ZERO, ZERO)
            S["side"] = side
            S["pelvis_l"] = add3(zero, side)                                             # :84
            S["knee_l"] = ik_solver(S["pelvis_l"], S["left_foot"], femur, tibia)
            S["pelvis_r"] = sub3(zero, side)                                             # :95
            S["knee_r"] = ik_solver(S["pelvis_r"], S["right_foot"], femur, tibia)
            lf, rf, kl, kr = S["left_foot"], S["right_foot"], S["knee_l"], S["knee_r"]
            S["left_toe"] = normalize((lf[1] - kl[1], kl[0] - lf[0], ZERO))              # :120
            S["right_toe"] = normalize((rf[1] - kr[1], kr[0] - rf[0], ZERO))             # :125
            S["wheel_pos"] = wheel_pos
        if len(_SCENES) > 64:
            _SCENES.clear()
        _SCENES[key] = S
    return _SCENES[key]


def sdf(build, u_time, px, py, pz, members=None):
    """sdf(P) (:38-144) of a build -> (distance, material id as float), arrays like px.  members: a dict that receives the
    distances of egg, legs, feet, bike and ground."""
    assert build in BUILDS, build
    S = scene(u_time)
    with np.errstate(all="ignore"):
        P = (_f(px), _f(py), _f(pz))
        r = mat_vec(S["rot_y"], P)
        p = (r[0] - ZERO, r[1] - F(0.5), r[2] - F(3.5))                                  # :40-41
        mat = _const(MAT_EGG, P[0])
        egg_y = F(0.65)
        if build != "oval":                                                             # :47-52
            egg_m = length3((p[0] - ZERO, p[1] - egg_y, p[2] - ZERO)) - F(0.475)
            egg_b = length3((p[0] - ZERO, p[1] - (egg_y - F(0.45)), p[2] - ZERO)) - F(0.25)
            egg_t = length3((p[0] - ZERO, p[1] - (egg_y + F(0.45)), p[2] - ZERO)) - F(0.25)
            egg = (op_blend(op_blend(egg_m, egg_b, HALF), egg_t, HALF), mat)
        else:                                                                           # :54-65
            s = F(1.55)
            scale = ((s, ZERO, ZERO), (ZERO, ONE, ZERO), (ZERO, ZERO, ONE))
            iscale = ((ONE / s, ZERO, ZERO), (ZERO, ONE / s, ZERO), (ZERO, ZERO, ONE))
            q = (p[0] - ZERO, p[1] - egg_y, p[2] - ZERO)
            egg = (length3(mat_vec(iscale, mat_vec(scale, q))) - F(0.475), mat)
        lf, rf, kl, kr, side = S["left_foot"], S["right_foot"], S["knee_l"], S["knee_r"], S["side"]
        zero = (ZERO, ZERO, ZERO)
        if build == "straight":                                                         # :86-93, :97-109
            left_a = sd_cylinder(add3(p, S["pelvis_l"]), sub3(kl, side), THICK)
            left_b = sd_cylinder(add3(p, kl), sub3(lf, kl), THICK)
            right_a = (sd_cylinder(add3(p, S["pelvis_r"]), add3(kr, side), THICK), mat)
            right_b = (sd_cylinder(add3(p, kr), sub3(rf, kr), THICK), mat)
            legs = op_add2((op_blend(left_a, left_b, F(.01)), mat), op_add2(right_a, right_b))
        else:                                                                           # :111-116
            legs = op_add2((sd_bezier_x(neg3(add3(zero, side)), neg3(kl), neg3(lf), p, THICK), mat),
                           (sd_bezier_x(neg3(sub3(zero, side)), neg3(kr), neg3(rf), p, THICK), mat))
        lt, rt = S["left_toe"], S["right_toe"]
        left_foot = (sd_cylinder(add3(p, lf), (lt[0] / F(8.), lt[1] / F(8.), lt[2] / F(8.)), THICK), mat)      # :120-123
        right_foot = (sd_cylinder(add3(p, rf), (rt[0] / F(8.), rt[1] / F(8.), rt[2] / F(8.)), THICK), mat)     # :125-128
        feet = op_add2(left_foot, right_foot)
        pw = add3(p, S["wheel_pos"])
        ring = np.sqrt(pw[0] * pw[0] + pw[1] * pw[1]) - ONE                              # sd_torus sdf.h:75-83
        bike = (np.sqrt(ring * ring + pw[2] * pw[2]) - F(.03), _const(MAT_BIKE, P[0]))
        ground = (dot((ZERO, ONE, ZERO), P) + (F(1.2) + F(0.5)), _const(MAT_GROUND, P[0]))   # :136-138
        if members is not None:
            members.update(egg=egg[0], legs=legs[0], feet=feet[0], bike=bike[0], ground=ground[0])
        _1 = op_add2(feet, bike)
        _2 = op_add2(egg, _1)
        _3 = op_add2(legs, _2)
        return op_add2(ground, _3)


def shadowmarch(build, u_time, ox, oy, oz):
    """shadowmarch({origin, (0, 1, 1)}) (:161-186), the statements of :171-182 in their order"""
    o = (_f(ox), _f(oy), _f(oz))
    dr = (ZERO, ONE, ONE)
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
            brk = ta > F(10.)
            hit = ~brk & (d < F(0.001))
            go = ~brk & ~hit
            dark[act[hit]] = True
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], F(15.) * d[go] / tn)
            act = act[go]
    return np.where(dark, F(0.1), umbra).astype(F)


# ---- the pixel -----------------------------------------------------------------------------------------------------------

def render_scene(build, u_time, ro, rd, parts=None):
    """render_scene (:190-231) for rays (ro, rd[3][n]) -> (rgb[n, 3], depth[n]).  parts: a dict that receives hit, p, mat, s."""
    n = rd[0].size
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(80):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k] + rd[k][act] * ta for k in range(3))
            d, m = sdf(build, u_time, *pi)
            brk = ta > F(15.)
            h = ~brk & (d < F(0.001))
            go = ~brk & ~h
            ih = act[h]
            hit[ih] = True
            mat[ih] = m[h].astype(np.int32)
            for k in range(3):
                p[k][ih] = pi[k][h]
            t[act[go]] = ta[go] + d[go]
            act = act[go]
        rgb = np.empty((n, 3), dtype=F)
        rgb[:] = (F(.1), F(.1), F(.7))              # background :10-13
        depth = np.full(n, F(-1e8), dtype=F)        # :188, fresh per invocation
        solid = hit & ((mat == MAT_EGG) | (mat == MAT_BIKE))
        depth[solid] = fmax(depth[solid], p[2][solid])                                   # :209-211
        s = np.ones(n, dtype=F)
        ig = np.flatnonzero(hit & (mat == MAT_GROUND))
        if ig.size:                                 # :214-222
            s[ig] = shadowmarch(build, u_time, p[0][ig] + ZERO * F(0.05), p[1][ig] + ONE * F(0.05), p[2][ig] + ONE * F(0.05))
        for m_id, col in COLORS.items():
            k = hit & (mat == m_id)
            rgb[k] = np.stack([col[c] * s[k] for c in range(3)], axis=1)
        other = hit & ~np.isin(mat, list(COLORS))
        rgb[other] = np.stack([ONE * s[other]] * 3, axis=1)
        if parts is not None:
            parts.update(hit=hit, p=np.stack(p, axis=1), mat=mat, s=s)
    return rgb, depth


def main_image(build, width, height, u_time, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    assert build in BUILDS, build
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), FOV)
    rd = get_primary_ray(pcx, pcy, EYE, LOOK_AT)
    rgb, depth = render_scene(build, u_time, EYE, rd, parts)
    with np.errstate(all="ignore"):                 # render :233-251
        x = np.abs(np.abs(pcx) - F(0.6)) - F(0.05)
        ts = clamp((x - ZERO) / (F(0.01) - ZERO), ZERO, ONE)
        bar_factor = ONE - (ts * ts) * (F(3.0) - TWO * ts)
        depth_factor = ONE - np.where(depth < ONE, ZERO, ONE).astype(F)
        a = (bar_factor * depth_factor)[:, None]
        col = np.abs(rgb * (ONE - a) + F(.6) * a)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = oracle().math("pow", np.ascontiguousarray(col).ravel(), F(1) / F(2.2)).reshape(col.shape)
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, rows=None, threads=8):
    """float32 [rows, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre); large frames go by row bands on `threads`
    threads (numpy and the oracle's math release the interpreter lock)"""
    ys = np.arange(height) if rows is None else np.asarray(list(rows))
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    band = max(1, 16384 // max(int(width), 1))
    bands = [ys[i:i + band] for i in range(0, len(ys), band)]
    scene(u_time)

    def one(b):
        return main_image(build, width, height, u_time, fx, (b.astype(F) + F(.5))[:, None])

    if len(bands) <= 1 or threads <= 1:
        return np.concatenate([one(b) for b in bands], axis=0)
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as ex:
        return np.concatenate(list(ex.map(one, bands)), axis=0)


fixture = functools.partial(builds_fixture, "egg")     # tests/golden/egg_builds/ decoded: tests/model_common.py
