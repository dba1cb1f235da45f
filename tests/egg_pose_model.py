"""numpy restatement of src/app_egg.h as shipped (`#define BEZIER`, the `#if 1` egg) under a POSE stated by the caller: the definition
of SBX_APP_EGG_POSE and sbx_egg_eval (include/sbx.h).  A pose is the block sbx_aux_egg_pose: eye, fov, look_at,
turn_deg, left_foot, femur, right_foot, tibia — the values the header derives from u_time or states as literals at :25, :26, :40,
:74, :77, :80, :81, :253; everything else stays its literal.

The primitives (ik_solver of src/IK.h, sd_bezier, sd_cylinder, op_blend, the matrices) are tests/egg_builds_model.py's, which is pinned
to the oracle; this module restates only what reads the pose: `scene_of`, sdf over a scene, sdf_normal, the two marches over arbitrary
rays, and the pixel with the block's camera.  It is pinned from two sides (tests/test_egg_pose_cpu.py): over `default_pose(u_time)` it
equals Oracle.render("egg") in every bit, and over the four poses of POSES it equals what the reference's own header rendered with
the eight literals replaced (tests/golden/egg_poses/, tools/make_golden_egg_poses.py).

binary32 step by step in the oracle's operation order, every value an explicit np.float32 (tests/model_common.py)."""
import os

import numpy as np

from tests.egg_builds_model import (COLORS, HALF, MAT_BIKE, MAT_EGG, MAT_GROUND, THICK, add3, clamp, ik_solver, mat_vec, neg3, op_blend,
                                    rotate_around_y, rotate_around_z, sd_bezier_x, sd_cylinder, sub3)
from tests.model_common import F, ONE, TWO, ZERO, _const, _f, dot, fmax, fmin, get_primary_ray, normalize, op_add2, oracle, point_cam, same_bits  # noqa: F401  (same_bits: for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE, POINTS = (64, 36), 64                          # the fixtures' frame and their number of seeded off-centre points
FIELDS = ("eye", "fov", "look_at", "turn_deg", "left_foot", "femur", "right_foot", "tibia")     # in the block's order, 16 floats
SHIPPED_EYE, SHIPPED_LOOK_AT = (.0, .25, 5.25), (.0, .25, .0)                                   # :25-26


def pose(left_foot, right_foot, turn_deg=0., femur=.8, tibia=.75, eye=SHIPPED_EYE, look_at=SHIPPED_LOOK_AT, fov=1.):
    """a pose from Python numbers, each rounded to binary32 once"""
    v3 = lambda v: tuple(F(c) for c in v)  # noqa: E731
    return dict(eye=v3(eye), fov=F(fov), look_at=v3(look_at), turn_deg=F(turn_deg), left_foot=v3(left_foot), femur=F(femur),
                right_foot=v3(right_foot), tibia=F(tibia))


def default_pose(u_time):
    """what setup_camera (:23-27) and sdf() (:40, :68-81) make of u_time: sbx_egg_pose_default"""
    with np.errstate(all="ignore"):
        t = F(u_time)
        wheel_pos = (ZERO, F(1.2), ZERO)
        pedal_radius, pedal_speed, pedal_off = F(0.3), F(400.), F(0.2)
        rot_z = rotate_around_z(-t * pedal_speed)                                        # :73, :76
        lf = add3(wheel_pos, mat_vec(rot_z, (ZERO, pedal_radius, pedal_off)))
        rf = add3(wheel_pos, mat_vec(rot_z, (ZERO, -pedal_radius, -pedal_off)))
        return dict(eye=tuple(map(F, SHIPPED_EYE)), fov=F(1.), look_at=tuple(map(F, SHIPPED_LOOK_AT)), turn_deg=t * F(-100.0),
                    left_foot=tuple(map(F, lf)), femur=F(0.8), right_foot=tuple(map(F, rf)), tibia=F(0.75))


def block(P):
    """the 16 floats of sbx_aux_egg_pose"""
    return np.array(list(P["eye"]) + [P["fov"]] + list(P["look_at"]) + [P["turn_deg"]] + list(P["left_foot"]) + [P["femur"]] +
                    list(P["right_foot"]) + [P["tibia"]], dtype=F)


def as_aux(P):
    """the pose as the ctypes block the Python binding takes (shaderbox_amd.EggPose)"""
    import ctypes

    import shaderbox_amd
    a = shaderbox_amd.EggPose()
    ctypes.memmove(ctypes.byref(a), block(P).tobytes(), 64)
    return a


# The fixture poses (tools/make_golden_egg_poses.py records them, check_conditions says what each must show):
#   stride  a turned rider seen from the side, both feet off the pedal circle
#   reach   the left foot beyond femur + tibia: a NaN knee, that leg and foot drop out of the union
#   bones   other bone lengths
#   inside  the camera within the bounding sphere of everything but the ground: no hot rectangle
POSES = {
    "stride": pose((.45, 1.25, .35), (-.3, 1.05, -.1), turn_deg=35., eye=(2., 1., 4.5), look_at=(0., 0., 0.), fov=.8),
    "reach": pose((.2, 1.7, .2), (0., 1., -.2)),
    "bones": pose((.3, 1.3, .2), (-.3, 1.1, -.2), femur=.6, tibia=.95),
    "inside": pose((0., 1.5, .2), (0., .9, -.2), turn_deg=90., eye=(3.5, -.2, .3), look_at=(3.5, 0., 0.), fov=1.),
}
POINT_SEEDS = {"stride": 101, "reach": 102, "bones": 103, "inside": 104}


def scene_of(P):
    """what sdf() (:38-144) computes before it reads its point, from the pose"""
    with np.errstate(all="ignore"):
        S = {"pose": P, "rot_y": rotate_around_y(P["turn_deg"])}                          # :40
        S["wheel_pos"] = (ZERO, F(1.2), ZERO)
        side = (ZERO, ZERO, F(0.2))                                                      # :71, :79
        zero = (ZERO, ZERO, ZERO)
        lf, rf = tuple(map(F, P["left_foot"])), tuple(map(F, P["right_foot"]))
        S["left_foot"], S["right_foot"], S["side"] = lf, rf, side
        S["pelvis_l"] = add3(zero, side)                                                 # :84
        S["knee_l"] = tuple(map(F, ik_solver(S["pelvis_l"], lf, P["femur"], P["tibia"])))
        S["pelvis_r"] = sub3(zero, side)                                                 # :95
        S["knee_r"] = tuple(map(F, ik_solver(S["pelvis_r"], rf, P["femur"], P["tibia"])))
        kl, kr = S["knee_l"], S["knee_r"]
        S["left_toe"] = normalize((lf[1] - kl[1], kl[0] - lf[0], ZERO))                  # :120
        S["right_toe"] = normalize((rf[1] - kr[1], kr[0] - rf[0], ZERO))                 # :125
    return S


def sdf(S, px, py, pz, members=None):
    """sdf(P) (:38-144) -> (distance, material id as float), arrays like px.  members: a dict that receives the distances of egg,
    legs, feet, bike and ground and `legs_win`, where the legs' member is the union's result."""
    with np.errstate(all="ignore"):
        P = (_f(px), _f(py), _f(pz))
        r = mat_vec(S["rot_y"], P)
        p = (r[0] - ZERO, r[1] - F(0.5), r[2] - F(3.5))                                  # :40-41
        mat = _const(MAT_EGG, P[0])
        egg_y = F(0.65)
        length3 = lambda v: np.sqrt(dot(v, v))  # noqa: E731
        egg_m = length3((p[0] - ZERO, p[1] - egg_y, p[2] - ZERO)) - F(0.475)             # :47-52
        egg_b = length3((p[0] - ZERO, p[1] - (egg_y - F(0.45)), p[2] - ZERO)) - F(0.25)
        egg_t = length3((p[0] - ZERO, p[1] - (egg_y + F(0.45)), p[2] - ZERO)) - F(0.25)
        egg = (op_blend(op_blend(egg_m, egg_b, HALF), egg_t, HALF), mat)
        lf, rf, kl, kr, side = S["left_foot"], S["right_foot"], S["knee_l"], S["knee_r"], S["side"]
        zero = (ZERO, ZERO, ZERO)
        legs = op_add2((sd_bezier_x(neg3(add3(zero, side)), neg3(kl), neg3(lf), p, THICK), mat),        # :111-116
                       (sd_bezier_x(neg3(sub3(zero, side)), neg3(kr), neg3(rf), p, THICK), mat))
        lt, rt = S["left_toe"], S["right_toe"]
        left_foot = (sd_cylinder(add3(p, lf), (lt[0] / F(8.), lt[1] / F(8.), lt[2] / F(8.)), THICK), mat)      # :120-123
        right_foot = (sd_cylinder(add3(p, rf), (rt[0] / F(8.), rt[1] / F(8.), rt[2] / F(8.)), THICK), mat)     # :125-128
        feet = op_add2(left_foot, right_foot)
        pw = add3(p, S["wheel_pos"])
        ring = np.sqrt(pw[0] * pw[0] + pw[1] * pw[1]) - ONE                              # sd_torus sdf.h:75-83
        bike = (np.sqrt(ring * ring + pw[2] * pw[2]) - F(.03), _const(MAT_BIKE, P[0]))
        ground = (dot((ZERO, ONE, ZERO), P) + (F(1.2) + F(0.5)), _const(MAT_GROUND, P[0]))   # :136-138
        _1 = op_add2(feet, bike)
        _2 = op_add2(egg, _1)
        _3 = op_add2(legs, _2)
        if members is not None:
            members.update(egg=egg[0], legs=legs[0], feet=feet[0], bike=bike[0], ground=ground[0],
                           legs_win=(legs[0] < _2[0]) & ~(ground[0] < _3[0]))
        return op_add2(ground, _3)


def sdf_normal(S, px, py, pz):
    """sdf_normal(p) (:146-157) -> [n, 3]; p + x is (p.x + dt, p.y + 0, p.z + 0), zero terms included"""
    with np.errstate(all="ignore"):
        p = (_f(px), _f(py), _f(pz))
        dt = F(0.05)
        g = []
        for ax in range(3):
            d = tuple(dt if k == ax else ZERO for k in range(3))
            g.append(sdf(S, p[0] + d[0], p[1] + d[1], p[2] + d[2])[0] - sdf(S, p[0] - d[0], p[1] - d[1], p[2] - d[2])[0])
        return np.stack(normalize(tuple(g)), axis=-1).astype(F)


def shadowmarch(S, o, dr):
    """shadowmarch({origin o[3][n], direction dr[3][n]}) (:161-186), the statements of :171-182 in their order"""
    o, dr = tuple(_f(c) for c in o), tuple(np.broadcast_to(_f(c), _f(o[0]).shape) for c in dr)
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
            d = sdf(S, *(o[k][act] + dr[k][act] * ta for k in range(3)))[0]
            brk = ta > F(10.)
            hit = ~brk & (d < F(0.001))
            go = ~brk & ~hit
            dark[act[hit]] = True
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], F(15.) * d[go] / tn)
            act = act[go]
    return np.where(dark, F(0.1), umbra).astype(F)


def render_scene(S, ro, rd, parts=None):
    """render_scene (:190-231) for rays (ro[3][n], rd[3][n]) -> (rgb[n, 3], depth[n]): `depth` (:188) starts at -max_dist for every
    ray.  parts: a dict that receives hit, p, mat, s, legs_win."""
    rd = tuple(_f(c).ravel() for c in rd)
    n = rd[0].size
    ro = tuple(np.broadcast_to(_f(c).ravel(), (n,)) for c in ro)
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    legs_win = np.zeros(n, dtype=bool)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(80):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k][act] + rd[k][act] * ta for k in range(3))
            mem = {}
            d, m = sdf(S, *pi, members=mem)
            brk = ta > F(15.)
            h = ~brk & (d < F(0.001))
            go = ~brk & ~h
            ih = act[h]
            hit[ih] = True
            mat[ih] = m[h].astype(np.int32)
            legs_win[ih] = mem["legs_win"][h]
            for k in range(3):
                p[k][ih] = pi[k][h]
            t[act[go]] = ta[go] + d[go]
            act = act[go]
        rgb = np.empty((n, 3), dtype=F)
        rgb[:] = (F(.1), F(.1), F(.7))              # background :10-13
        depth = np.full(n, F(-1e8), dtype=F)        # :188
        solid = hit & ((mat == MAT_EGG) | (mat == MAT_BIKE))
        depth[solid] = fmax(depth[solid], p[2][solid])                                   # :209-211
        s = np.ones(n, dtype=F)
        ig = np.flatnonzero(hit & (mat == MAT_GROUND))
        if ig.size:                                 # :214-222, sh_dir = (0, 1, 1)
            s[ig] = shadowmarch(S, (p[0][ig] + ZERO * F(0.05), p[1][ig] + ONE * F(0.05), p[2][ig] + ONE * F(0.05)), (ZERO, ONE, ONE))
        for m_id, col in COLORS.items():
            k = hit & (mat == m_id)
            rgb[k] = np.stack([col[c] * s[k] for c in range(3)], axis=1)
        if parts is not None:
            parts.update(hit=hit, p=np.stack(p, axis=1), mat=mat, s=s, legs_win=legs_win)
    return rgb, depth


def finish(rgb, depth, pcx):
    """render's bars and abs (:233-251), then main.h's linear_to_srgb and alpha 1 -> [n, 4]"""
    with np.errstate(all="ignore"):
        x = np.abs(np.abs(_f(pcx)) - F(0.6)) - F(0.05)
        ts = clamp((x - ZERO) / (F(0.01) - ZERO), ZERO, ONE)
        bar_factor = ONE - (ts * ts) * (F(3.0) - TWO * ts)
        depth_factor = ONE - np.where(depth < ONE, ZERO, ONE).astype(F)
        a = (bar_factor * depth_factor)[:, None]
        col = np.abs(rgb * (ONE - a) + F(.6) * a)
    out = np.ones((rgb.shape[0], 4), dtype=F)       # main.h:52
    out[:, :3] = oracle().math("pow", np.ascontiguousarray(col).ravel(), F(1) / F(2.2)).reshape(col.shape)
    return out


def primary_rays(P, width, height, fx, fy):
    """(point_cam.x, ro[3], rd[3][n]) of the block's camera at fragCoords (fx, fy), flat"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), P["fov"])
    return pcx, P["eye"], get_primary_ray(pcx, pcy, P["eye"], P["look_at"])


def main_image(S, width, height, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    shape = np.broadcast(_f(fx), _f(fy)).shape
    pcx, ro, rd = primary_rays(S["pose"], width, height, fx, fy)
    rgb, depth = render_scene(S, ro, rd, parts)
    return finish(rgb, depth, pcx).reshape(shape + (4,))


def frame(S, width, height, parts=None):
    """float32 [H, W, 4] (row 0 = bottom; fragCoord = pixel centre)"""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(S, width, height, fx, fy, parts)


def points(S, width, height, frag):
    frag = np.asarray(frag, dtype=F).reshape(-1, 2)
    return main_image(S, width, height, frag[:, 0], frag[:, 1])


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a fixture"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/egg_poses/<name>_WxH.npz: pose [16], frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    return np.load(os.path.join(GOLDEN, "egg_poses", "%s_%dx%d.npz" % (name, SIZE[0], SIZE[1])))


def shares(S, width, height):
    """the shares of the frame's pixels that check_conditions reads, and the frame"""
    parts = {}
    f = frame(S, width, height, parts)
    n = float(width * height)
    hit, mat = parts["hit"], parts["mat"]
    ground = hit & (mat == MAT_GROUND)
    return dict(egg=(hit & (mat == MAT_EGG)).sum() / n, legs=(hit & parts["legs_win"]).sum() / n, bike=(hit & (mat == MAT_BIKE)).sum() / n,
                ground=ground.sum() / n, background=(~hit).sum() / n, shadowed=(ground & (parts["s"] < ONE)).sum() / n), f


def check_conditions(all_shares, frames):
    """The conditions under which the fixtures say something, over {name: shares(...)[0]} and {name: frame}: asserted by the tool that
    records them and again of the committed files.  Conditions, not measurements."""
    assert set(all_shares) == set(POSES) == set(frames)
    for name in ("stride", "reach", "bones"):
        s = all_shares[name]
        assert s["egg"] >= .05 and s["legs"] >= .005 and s["bike"] >= .01 and s["ground"] >= .30 and s["background"] >= .30 and \
            s["shadowed"] >= .015, (name, s)
    s = all_shares["inside"]
    assert s["legs"] >= .10 and s["bike"] >= .02 and s["ground"] == 0, ("inside", s)
    assert np.isnan(np.array(scene_of(POSES["reach"])["knee_l"])).any(), "reach: the left knee is a NaN"
    assert not np.isnan(frames["reach"]).any(), "reach: the frame holds no NaN"
    for f in frames.values():
        assert (f[..., 3] == 1).all()

