"""numpy restatement of src/app_vinyl.h as shipped (SHADERTOY undefined, the C++ build's 60 march steps) over a DECK stated by the
caller: the definition of SBX_APP_VINYL_DECK and sbx_vinyl_eval (include/sbx.h).  A deck is the block
sbx_aux_vinyl_deck: eye, fov, look_at, platter_deg, sun_dir, platter_tilt_deg, the five base colours with arm_tilt_deg, ro_spec, a_x,
a_y and shininess beside them — the values the header derives from u_time or states as literals at :45-53, :61, :62, :141-142,
:284-285, :327-329, :375, :419, :428 and :460; everything else stays its literal.

The primitives (sdf_platter, sdf_tonearm, the matrices, saw, pulse) are tests/vinyl_builds_model.py's, which is pinned to the oracle;
this module restates only what reads the deck: `scene_of`, sdf over a scene, sdf_normal, sdf_shadow over arbitrary rays, illuminate
with the block's colours and constants, render over arbitrary rays, and the pixel with the block's camera.  It is pinned from two sides
(tests/test_vinyl_deck_cpu.py): over `default_deck(u_time)` it equals Oracle.render("vinyl") in every bit, and over the decks of DECKS
it equals what the reference's own header rendered with the literals replaced (tests/golden/vinyl_decks/,
tools/make_golden_vinyl_decks.py).

binary32 step by step in the oracle's operation order, every value an explicit np.float32 (tests/model_common.py)."""
import os

import numpy as np

from tests import vinyl_builds_model as V
from tests.egg_builds_model import length3
from tests.model_common import F, ONE, TWO, ZERO, _f, cross, dot, fmax, fmin, get_primary_ray, normalize, op_add2, oracle, point_cam, same_bits  # noqa: F401  (same_bits: for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE, POINTS = (64, 36), 64                          # the fixtures' frame and their number of seeded off-centre points
# the block's order, 32 floats: a vec3 and a scalar per row
FIELDS = ("eye", "fov", "look_at", "platter_deg", "sun_dir", "platter_tilt_deg", "groove_color", "arm_tilt_deg", "dead_wax_color", "ro_spec",
          "label_color", "a_x", "logo_color", "a_y", "shiny_color", "shininess")
CAMERA_FIELDS = ("eye", "fov", "look_at")
SHIPPED_EYE, SHIPPED_LOOK_AT = V.CAMERA["default"]                                              # :61-62
COLOR_OF = {V.MAT_GROOVE: "groove_color", V.MAT_DEAD_WAX: "dead_wax_color", V.MAT_LABEL: "label_color", V.MAT_LOGO: "logo_color",
            V.MAT_SHINY: "shiny_color"}
# which materials' pixels read a field (None: the geometry or the light reads it — any hit pixel, and for the angles any pixel)
READERS = {"fov": None, "platter_deg": None, "platter_tilt_deg": None, "arm_tilt_deg": None, "sun_dir": (1, 2, 3, 4, 5),
           "groove_color": (1,), "dead_wax_color": (2,), "label_color": (3,), "logo_color": (4,), "shiny_color": (5,),
           "ro_spec": (1, 2), "a_x": (1, 2), "a_y": (1, 2), "shininess": (3, 4, 5)}


def _v3(v):
    return tuple(F(c) for c in v)


def default_deck(u_time):
    """what app_vinyl.h makes of u_time: sbx_vinyl_deck_default"""
    with np.errstate(all="ignore"):
        t = F(u_time)
        o = oracle()
        s1 = o.math("sin", _f(t).reshape(1))[0]
        s2 = o.math("sin", _f(t * F(3.6758)).reshape(1))[0]
        D = dict(eye=_v3(SHIPPED_EYE), fov=F(1.), look_at=_v3(SHIPPED_LOOK_AT), platter_deg=t * F(200.),
                 sun_dir=_v3(V.constants()["sun_dir"]), platter_tilt_deg=s1 * F(.1), arm_tilt_deg=s2 * F(.1),
                 ro_spec=F(.0725), a_x=F(.025), a_y=F(.5), shininess=F(50.))
        for m, name in COLOR_OF.items():
            D[name] = _v3(V.BASE_COLOR[m])
    return D


def deck(u_time=0., **fields):
    """default_deck(u_time) with the named fields replaced, each value rounded to binary32 once"""
    D = default_deck(u_time)
    for k, v in fields.items():
        assert k in FIELDS, k
        D[k] = _v3(v) if isinstance(D[k], tuple) else F(v)
    return D


def block(D):
    """the 32 floats of sbx_aux_vinyl_deck"""
    out = []
    for k in FIELDS:
        out += list(D[k]) if isinstance(D[k], tuple) else [D[k]]
    return np.array(out, dtype=F)


def as_aux(D):
    """the deck as the ctypes block the Python binding takes (shaderbox_amd.VinylDeck)"""
    import ctypes

    import shaderbox_amd
    a = shaderbox_amd.VinylDeck()
    ctypes.memmove(ctypes.byref(a), block(D).tobytes(), 128)
    return a


# The fixture decks (tools/make_golden_vinyl_decks.py records them, check_conditions says what each must show):
#   scratch   another platter angle, both tilts at several degrees
#   coloured  all five colours and the four shading constants changed
#   dusk      a low, un-normalised sun from the other side
#   far       an eye beyond the tame domain (sbx_vinyl.h): the frame must take the plain form; 60 steps end in the air, all background
DECKS = {
    "scratch": deck(platter_deg=-77.5, platter_tilt_deg=4., arm_tilt_deg=-3.),
    "coloured": deck(.37, groove_color=(.03, .01, .02), dead_wax_color=(.1, .02, .02), label_color=(.1, .6, .3), logo_color=(.8, .1, 0.),
                     shiny_color=(.9, .6, .2), ro_spec=.12, a_x=.05, a_y=.3, shininess=12.),
    "dusk": deck(2.5, sun_dir=(1.5, .6, 1.)),
    "far": deck(.37, eye=(0., 15000., 15000.), look_at=(0., 0., 0.)),
}
POINT_SEEDS = {"scratch": 201, "coloured": 202, "dusk": 203, "far": 204}
SHIPPED_CAMERA = ("scratch", "coloured", "dusk")


def scene_of(D):
    """what render (:419-428) and sdf_tonearm (:141-142) compute before they read a point, from the deck"""
    with np.errstate(all="ignore"):
        return {"deck": D, "platter_rot": V.mat_mat(V.rotate_around_y(D["platter_deg"]), V.rotate_around_x(D["platter_tilt_deg"])),
                "wobble": V.rotate_around_x(D["arm_tilt_deg"])}


def sdf(S, px, py, pz):
    """sdf(pos) (:251-259) -> (distance, material id as float), arrays like px"""
    with np.errstate(all="ignore"):
        pos = (_f(px), _f(py), _f(pz))
        plat = V.sdf_platter(V.vec_mat(pos, S["platter_rot"]))
        arm = V.sdf_tonearm(S, pos)
        return op_add2(plat, arm)


def sdf_normal(S, p):
    """sdf_normal(p) (:261-272) -> a tuple of three arrays; p + x is (p.x + dt, p.y + 0, p.z + 0), zero terms included"""
    with np.errstate(all="ignore"):
        p = tuple(_f(c) for c in p)
        dt = F(0.001)
        g = []
        for ax in range(3):
            d = tuple(dt if k == ax else ZERO for k in range(3))
            g.append(sdf(S, p[0] + d[0], p[1] + d[1], p[2] + d[2])[0] - sdf(S, p[0] - d[0], p[1] - d[1], p[2] - d[2])[0])
        return normalize(tuple(g))


def sdf_shadow(S, o, dr):
    """sdf_shadow({origin o[3][n], direction dr[3]}) (:381-405), the statements of :391-401 in their order"""
    o = tuple(_f(c) for c in o)
    dr = tuple(np.broadcast_to(_f(c), o[0].shape) for c in dr)
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
            brk = ta > F(5.)
            hit = ~brk & (d < F(.005))
            go = ~brk & ~hit
            dark[act[hit]] = True
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], F(16.) * d[go] / tn)
            act = act[go]
    return np.where(dark, F(.05), umbra).astype(F)


def to_int(x):
    """int() of a material id given as a float: toward zero, saturating at the ends of int, 0 for a NaN (include/sbx.h)"""
    x = _f(x)
    with np.errstate(all="ignore"):
        c = np.clip(np.where(np.isnan(x), ZERO, x).astype(np.float64), -2147483648., 2147483520.)
    return np.trunc(c).astype(np.int64).astype(np.int32)


def illuminate(S, eye, p, mat):
    """illuminate(eye, hit) (:287-379) for hits p[3][n] of material ids mat[n] (ints) seen from eye[3] (scalars or [n]) -> rgb[n, 3]"""
    D = S["deck"]
    mat = np.asarray(mat)
    n = mat.size
    p = tuple(_f(c) for c in p)
    eye = tuple(np.broadcast_to(_f(c), (n,)) for c in eye)
    out = np.zeros((n, 3), dtype=F)
    with np.errstate(all="ignore"):
        L = D["sun_dir"]
        Vv = normalize(tuple(eye[k] - p[k] for k in range(3)))
        base = np.zeros((n, 3), dtype=F)             # an unset slot is zero
        base[mat == 0] = V.BASE_COLOR[0]             # mat_debug stays the literal
        for m_id, name in COLOR_OF.items():
            base[mat == m_id] = D[name]
        plat = (mat == V.MAT_GROOVE) | (mat == V.MAT_DEAD_WAX)
        g = np.flatnonzero(plat)
        if g.size:                                  # :300-353
            rot = S["platter_rot"]
            ho = V.vec_mat(tuple(p[k][g] for k in range(3)), rot)
            Lr = V.vec_mat(L, rot)
            Vr = V.vec_mat(tuple(Vv[k][g] for k in range(3)), rot)
            r = length3(ho)
            B = (ho[0] / r, ho[1] / r, ho[2] / r)
            N = [np.zeros(g.size, dtype=F), np.ones(g.size, dtype=F), np.zeros(g.size, dtype=F)]
            mg = mat[g]
            is_g = mg == V.MAT_GROOVE
            if is_g.any():
                xyz = np.stack([ho[k] * F(2.456) for k in range(3)], axis=1)
                rr = r + F(.07575) * oracle().noise("noise_iq", np.ascontiguousarray(xyz))[:, 0]
                s = V.pulse(rr * F(24.))
                k = is_g & (s > ZERO)
                Nn = normalize((N[0] + B[0], N[1] + B[1], N[2] + B[2]))
                d2 = TWO * ((ZERO * Nn[0] + ONE * Nn[1]) + ZERO * Nn[2])                  # reflect(N, (0, 1, 0)) util_optics.h:17-22
                Nr = (Nn[0] - d2 * ZERO, Nn[1] - d2 * ONE, Nn[2] - d2 * ZERO)
                for c in range(3):
                    N[c] = np.where(k, Nr[c], N[c])
            is_d = mg == V.MAT_DEAD_WAX
            if is_d.any():
                s = V.saw(r * F(4.))
                f = np.where(s > F(.9), ONE, ZERO).astype(F)
                Nd = normalize((N[0] + B[0] * f, N[1] + B[1] * f, N[2] + B[2] * f))
                for c in range(3):
                    N[c] = np.where(is_d, Nd[c], N[c])
            N = tuple(N)
            T = cross(B, N)
            ro_diff, ro_spec, a_x, a_y = F(1.), D["ro_spec"], D["a_x"], D["a_y"]         # :326-329
            Hh = normalize((Vr[0] + Lr[0], Vr[1] + Lr[1], Vr[2] + Lr[2]))
            dotLN = dot(Lr, N)
            dmax = fmax(np.zeros_like(dotLN), dotLN)
            spec_a = ro_spec / np.sqrt(dotLN * dot(Vr, N))
            spec_b = ONE / (F(4.) * V.PI * a_x * a_y)
            ht = dot(Hh, T) / a_x
            hb = dot(Hh, B) / a_y
            spec_c = F(-2.) * (ht * ht + hb * hb) / (ONE + dot(Hh, N))
            spec = ONE * spec_a * spec_b * oracle().math("exp", np.ascontiguousarray(spec_c))
            for c in range(3):
                out[g, c] = base[g, c] * (ro_diff / V.PI) * dmax + spec
        e = np.flatnonzero(~plat)
        if e.size:                                  # :354-378
            nrm = sdf_normal(S, tuple(p[k][e] for k in range(3)))
            dLn = dot(L, nrm)
            diff = fmax(np.zeros_like(dLn), dLn)
            Ve = tuple(Vv[k][e] for k in range(3))
            Hh = normalize((Ve[0] + L[0], Ve[1] + L[1], Ve[2] + L[2]))
            dHn = dot(Hh, nrm)
            spec = oracle().math("pow", np.ascontiguousarray(fmax(np.zeros_like(dHn), dHn)), D["shininess"]) * ONE       # :375
            for c in range(3):
                out[e, c] = base[e, c] * diff + spec
    return out


def render(S, ro, rd, parts=None):
    """render (:407-458) for rays (ro[3] scalars or [n], rd[3][n]) -> (rgb[n, 3] LINEAR, t[n] as it stands where render returns,
    mat[n]: the hit's material id as a float, 0 for the background).  parts: a dict that receives hit, p, mat, sh, lit."""
    rd = tuple(_f(c).ravel() for c in rd)
    n = rd[0].size
    ro = tuple(np.broadcast_to(_f(c).ravel(), (n,)) for c in ro)
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    sun = S["deck"]["sun_dir"]
    with np.errstate(all="ignore"):
        for _ in range(V.STEPS):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k][act] + rd[k][act] * ta for k in range(3))
            d, m = sdf(S, *pi)
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
            sh[ih] = sdf_shadow(S, tuple(ph[k] + sun[k] * F(0.05) for k in range(3)), sun)      # :445-450
            lit[ih] = illuminate(S, tuple(ro[k][ih] for k in range(3)), ph, mat[ih])
            rgb[ih] = lit[ih] * sh[ih][:, None]
        if parts is not None:
            parts.update(hit=hit, p=np.stack(p, axis=1), mat=mat, sh=sh, lit=lit)
    return rgb, t, np.where(hit, mat, 0).astype(F)


def finish(rgb):
    """main.h's linear_to_srgb and alpha 1 -> [n, 4]"""
    out = np.ones((rgb.shape[0], 4), dtype=F)       # main.h:52
    with np.errstate(all="ignore"):
        out[:, :3] = oracle().math("pow", np.ascontiguousarray(rgb).ravel(), F(1) / F(2.2)).reshape(rgb.shape)
    return out


def primary_rays(D, width, height, fx, fy):
    """(ro[3], rd[3][n]) of the block's camera at fragCoords (fx, fy), flat"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), D["fov"])
    return D["eye"], get_primary_ray(pcx, pcy, D["eye"], D["look_at"])


def main_image(S, width, height, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    shape = np.broadcast(_f(fx), _f(fy)).shape
    ro, rd = primary_rays(S["deck"], width, height, fx, fy)
    return finish(render(S, ro, rd, parts)[0]).reshape(shape + (4,))


def frame_coords(width, height):
    return (np.arange(width, dtype=F) + F(.5))[None, :], (np.arange(height, dtype=F) + F(.5))[:, None]


def frame(S, width, height, parts=None):
    """float32 [H, W, 4] (row 0 = bottom; fragCoord = pixel centre)"""
    fx, fy = frame_coords(width, height)
    return main_image(S, width, height, fx, fy, parts)


def points(S, width, height, frag):
    frag = np.asarray(frag, dtype=F).reshape(-1, 2)
    return main_image(S, width, height, frag[:, 0], frag[:, 1])


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a fixture"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/vinyl_decks/<name>_WxH.npz: deck [32], frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    return np.load(os.path.join(GOLDEN, "vinyl_decks", "%s_%dx%d.npz" % (name, SIZE[0], SIZE[1])))


def shares(S, width, height):
    """what check_conditions reads of a frame — the share of its pixels per material, the logo's pixel count, the hit mask — and the frame"""
    parts = {}
    f = frame(S, width, height, parts)
    n = float(width * height)
    hit, mat = parts["hit"], parts["mat"]
    of = lambda m: (hit & (mat == m)).sum()  # noqa: E731
    return dict(groove=of(V.MAT_GROOVE) / n, dead_wax=of(V.MAT_DEAD_WAX) / n, label=of(V.MAT_LABEL) / n, shiny=of(V.MAT_SHINY) / n,
                logo_pixels=int(of(V.MAT_LOGO)), hit=hit.reshape(height, width), mat=np.where(hit, mat, 0).reshape(height, width)), f


def differing(a, b):
    """the pixels at which two frames differ in a bit"""
    return (~same_bits(a, b)).any(axis=-1)


def check_conditions(all_shares, frames, default_shares, default_frame):
    """The conditions under which the fixtures say something, over {name: shares(...)[0]}, {name: frame} and the same of the default block
    (default_deck(0.)): asserted by the tool that records them and again of the committed files.  Conditions, not measurements."""
    assert set(all_shares) == set(DECKS) == set(frames)
    for name in SHIPPED_CAMERA:
        s = all_shares[name]
        assert s["groove"] >= .30 and s["dead_wax"] >= .05 and s["label"] >= .02 and s["shiny"] >= .03 and s["logo_pixels"] >= 8, (name, s)
    for name, f in frames.items():
        hit = all_shares[name]["hit"] | default_shares["hit"]            # hit in either frame
        assert differing(f, default_frame).sum() * 10 >= hit.sum() > 0, (name, "differs from the default block's frame in too few pixels")
        assert (f[..., 3] == 1).all()
    assert not all_shares["far"]["hit"].any(), "far: 60 steps end in the air"


def single_field_decks():
    """for each of the 14 fields beside the camera's position (eye, look_at), default_deck(0.) with that field alone changed"""
    other = dict(fov=.9, platter_deg=33., platter_tilt_deg=2.5, arm_tilt_deg=3., sun_dir=(.5, .8, .2), groove_color=(.02, .03, .01),
                 dead_wax_color=(.02, .08, .05), label_color=(.2, .5, .4), logo_color=(.6, 0., .1), shiny_color=(.3, .7, .6), ro_spec=.1, a_x=.04,
                 a_y=.25, shininess=9.)
    assert set(other) == set(FIELDS) - {"eye", "look_at"} == set(READERS) and len(other) == 14
    return {k: deck(0., **{k: v}) for k, v in other.items()}
