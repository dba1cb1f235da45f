"""SBX_APP_RAYTRACER_SCENE (include/sbx.h): src/app_raytracer.h's render (:88-136) over a scene, a camera and a FOV of the caller's,
restated in numpy binary32 in the oracle's operation order.  The definition of that app.

tests/raytracer_builds_model.py already takes the scene as a dictionary S — nothing in its trace, fresnel_factor, material and the two
lighting models knows the Cornell box — so those are imported as they are; what this file adds is what the four builds have as
compile-time text and the scene app has as values of its block: the bounce count (:96), the lighting model (:61), the shadow ray
(:107), the light's type (light.h:18-27) and the ambient colour (light.h:16).

    S = dict(planes=[((nx, ny, nz), d, material id)], spheres=[((ox, oy, oz), radius, material id)],      array order
             base=float32[8, 3], rough=float32[8], ior=float32[8], refl=float32[8],                          the material slots
             light=(x, y, z), light_type=1 | 2, lighting=0 | 1, shadow=0 | 1, bounces=1..8, ambient=(r, g, b),
             eye=(x, y, z), look_at=(x, y, z), fov=float32)

As in the reference: a sphere whose material equals mat_to_ignore is not intersected — material 0 in the shadow trace (mat_debug, :116)
and material -1 in every trace (mat_invalid, :97); planes are never skipped.

Pinned from two sides (tests/test_raytracer_scene_cpu.py): over the Cornell block it equals the oracle's `raytracer` in every bit, and
over the scenes of tests/golden/raytracer_scenes.json it equals what the reference's own headers rendered with those scenes written
into them (tools/make_golden_raytracer_scenes.py, tests/golden/raytracer_scenes/)."""
import json
import os

import numpy as np

from tests.model_common import F, ONE, TWO, ZERO, _f, dot, get_primary_ray, point_cam, same_bits  # noqa: F401
from tests.raytracer_builds_model import BIAS, MAX_DIST, _math, fresnel_factor, illum_blinn_phong, illum_cook_torrance, material, normalize, trace

LIGHT_POINT, LIGHT_DIR = 1, 2                       # light.h:5-6
SPHERE_TAG = 1 << 20                                # first_kind(): material ids that no plane of a test scene carries


def illuminate(S, eye, mat, nor, org):              # :46-68 -> (colour, L)
    base, rough, ior, _ = material(S, mat)
    V = normalize([eye[k] - org[k] for k in range(3)])
    if S["light_type"] == LIGHT_DIR:                # get_light_direction light.h:18-27: light.L as given
        L = [np.broadcast_to(F(S["light"][k]), org[k].shape) for k in range(3)]
    else:
        L = normalize([S["light"][k] - org[k] for k in range(3)])
    lit = illum_blinn_phong(V, L, nor, base) if S["lighting"] else illum_cook_torrance(V, L, nor, base, rough, ior)
    debug = mat == 0                                # mat_debug: materials[mat_debug].base_color
    return [np.where(debug, S["base"][0, k], F(S["ambient"][k]) + lit[k]) for k in range(3)], L


def render(S, eye, rd, masks=None):                 # :88-136
    """the linear colour of the rays (eye, rd), rd three float32 arrays.  masks: a dict that receives, per ray,
        first_kind  0 background, 1 a plane, 2 a sphere: what the primary ray hit
        first_mat   that hit's material id (-1: none)
        lit         the first hit is no mat_debug hit and dot(normal, L) > 0
        shadowed    the shadow test of bounce 0 darkened the pixel
        depth       the number of raytrace_iteration calls of the bounce loop that found a hit (0 = background)"""
    n = rd[0].shape
    eye = [F(v) for v in eye]
    color = [np.zeros(n, dtype=F) for _ in range(3)]
    accum = [np.ones(n, dtype=F) for _ in range(3)]
    ro = [np.full(n, eye[k], dtype=F) for k in range(3)]
    rd = [np.asarray(v, dtype=F) for v in rd]
    active = np.ones(n, dtype=bool)
    depth = np.zeros(n, dtype=np.int32)
    shadowed = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(int(S["bounces"])):
            t, mat, nor, org = trace(S, ro, rd, -1)
            miss = active & (t >= MAX_DIST)
            live = active & ~miss
            depth = depth + live
            f = fresnel_factor(ONE, ONE, dot(nor, [-rd[k] for k in range(3)]))
            ill, L = illuminate(S, eye, mat, nor, org)             # the primary origin on every bounce (:105)
            if i == 0 and masks is not None:
                tagged = dict(S, spheres=[(o, r, SPHERE_TAG + j) for j, (o, r, m) in enumerate(S["spheres"]) if m != -1])
                kind = trace(tagged, ro, rd, -1)[1] >= SPHERE_TAG
                masks.update(first_kind=np.where(miss, 0, np.where(kind, 2, 1)).astype(np.int32), first_mat=np.where(live, mat, -1),
                             lit=live & (mat != 0) & (dot(nor, L) > ZERO))
            for k in range(3):
                color[k] = np.where(miss, color[k] + accum[k] * ZERO, color[k])              # background :13-16
                color[k] = np.where(live, color[k] + ((ONE - f) * accum[k]) * ill[k], color[k])
            if i == 0 and S["shadow"]:                  # shadow ray :108-121: light.L - hit.origin whatever the light's type (:109)
                line = [S["light"][k] - org[k] for k in range(3)]
                sdir = normalize(line)
                st = trace(S, [org[k] + sdir[k] * BIAS for k in range(3)], sdir, 0)[0]
                shadowed = live & (st < np.sqrt(dot(line, line)))
                for k in range(3):
                    color[k] = np.where(shadowed, color[k] * F(0.1), color[k])
            refl = live & (material(S, mat)[3] > ZERO)
            s = TWO * dot(rd, nor)                      # reflect(hit.normal, ray.direction): arguments swapped in the reference (:127)
            rdir = normalize([nor[k] - s * rd[k] for k in range(3)])
            for k in range(3):
                accum[k] = np.where(refl, accum[k] * f, accum[k])
                ro[k] = np.where(refl, org[k] + rdir[k] * BIAS, ro[k])
                rd[k] = np.where(refl, rdir[k], rd[k])
            active = refl
    if masks is not None:
        masks.update(shadowed=shadowed, depth=depth)
    return color


def main_image(S, eye, look_at, fov, w, h, fx, fy, masks=None):
    """fragColor at fragCoords (fx, fy) of a w x h frame -> float32 [..., 4]; masks as render's, in the shape of fx"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(w, h, fx.ravel(), fy.ravel(), F(fov))
    rd = get_primary_ray(pcx, pcy, eye, look_at)
    color = render(S, eye, rd, masks)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = _math("pow", color[k], F(1) / F(2.2))
    if masks is not None:
        for k in masks:
            masks[k] = masks[k].reshape(shape)
    return out.reshape(shape + (4,))


def frame(S, w, h, masks=None):
    """float32 [h, w, 4] of the frame (row 0 = bottom; fragCoord = pixel centre) from S's own eye, look_at and fov"""
    fx = (np.arange(w, dtype=F) + F(.5))[None, :]
    fy = (np.arange(h, dtype=F) + F(.5))[:, None]
    return main_image(S, S["eye"], S["look_at"], S["fov"], w, h, fx, fy, masks)


def points(S, w, h, pts, masks=None):
    pts = np.asarray(pts, dtype=F)
    return main_image(S, S["eye"], S["look_at"], S["fov"], w, h, pts[:, 0], pts[:, 1], masks)


def from_block(a):
    """shaderbox_amd.RaytracerScene -> S: the first n_planes / n_spheres entries, every value the block's binary32"""
    v3 = lambda p: tuple(F(p[k]) for k in range(3))  # noqa: E731
    m = a.materials
    return dict(planes=[(v3(p.direction), F(p.distance), int(p.material)) for p in a.planes[:a.n_planes]],
                spheres=[(v3(s.origin), F(s.radius), int(s.material)) for s in a.spheres[:a.n_spheres]],
                base=np.array([[m[i].base_color[k] for k in range(3)] for i in range(8)], dtype=F),
                rough=np.array([m[i].roughness for i in range(8)], dtype=F), ior=np.array([m[i].ior for i in range(8)], dtype=F),
                refl=np.array([m[i].reflectivity for i in range(8)], dtype=F),
                metallic=np.array([m[i].metallic for i in range(8)], dtype=F), transl=np.array([m[i].translucency for i in range(8)], dtype=F),
                light=v3(a.light_L), light_color=v3(a.light_color), light_type=int(a.light_type), lighting=int(a.lighting),
                shadow=int(a.shadow), bounces=int(a.bounces), ambient=v3(a.ambient), eye=v3(a.eye), look_at=v3(a.look_at), fov=F(a.fov))


def to_block(S):
    """S -> shaderbox_amd.RaytracerScene (metallic, translucency and light_color where S carries them, else 0 / 0 / (1, 1, 1))"""
    import shaderbox_amd
    a = shaderbox_amd.RaytracerScene()
    put = lambda d, v: d.__setitem__(slice(0, 3), [float(F(x)) for x in v])  # noqa: E731
    put(a.eye, S["eye"]), put(a.look_at, S["look_at"]), put(a.light_L, S["light"]), put(a.ambient, S["ambient"])
    put(a.light_color, S.get("light_color", (1.0, 1.0, 1.0)))
    a.fov, a.bounces, a.light_type, a.lighting, a.shadow = float(F(S["fov"])), int(S["bounces"]), int(S["light_type"]), int(S["lighting"]), int(S["shadow"])
    a.n_planes, a.n_spheres = len(S["planes"]), len(S["spheres"])
    for i in range(8):
        m = a.materials[i]
        put(m.base_color, S["base"][i])
        m.roughness, m.ior, m.reflectivity = float(S["rough"][i]), float(S["ior"][i]), float(S["refl"][i])
        m.metallic = float(S["metallic"][i]) if "metallic" in S else 0.0
        m.translucency = float(S["transl"][i]) if "transl" in S else 0.0
    for i, (n, d, mat) in enumerate(S["planes"]):
        put(a.planes[i].direction, n)
        a.planes[i].distance, a.planes[i].material = float(F(d)), int(mat)
    for i, (o, r, mat) in enumerate(S["spheres"]):
        put(a.spheres[i].origin, o)
        a.spheres[i].radius, a.spheres[i].material = float(F(r)), int(mat)
    return a


def nan_pixels(a):
    return int(np.isnan(a).any(axis=-1).sum())


# ---- the fixture scenes: tests/golden/raytracer_scenes.json (settings only) and tests/golden/raytracer_scenes/<name>_64x36.npz ------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def scene_table():
    """the JSON as it is: {"size": [w, h], "points": n, "scenes": [...]}, every float a hex-float string"""
    with open(os.path.join(GOLDEN, "raytracer_scenes.json")) as f:
        return json.load(f)


def scene_of(entry):
    """one entry of the table -> S"""
    x = lambda s: F(float.fromhex(s))  # noqa: E731
    v3 = lambda p: tuple(x(c) for c in p)  # noqa: E731
    m = entry["materials"]
    assert len(m) == 8
    col = lambda key: np.array([x(m[i][key]) for i in range(8)], dtype=F)  # noqa: E731
    return dict(planes=[(v3(p["direction"]), x(p["distance"]), int(p["material"])) for p in entry["planes"]],
                spheres=[(v3(s["origin"]), x(s["radius"]), int(s["material"])) for s in entry["spheres"]],
                base=np.array([v3(m[i]["base_color"]) for i in range(8)], dtype=F), rough=col("roughness"), ior=col("ior"),
                refl=col("reflectivity"), metallic=col("metallic"), transl=col("translucency"),
                light=v3(entry["light_L"]), light_color=v3(entry["light_color"]), light_type=int(entry["light_type"]),
                lighting=int(entry["lighting"]), shadow=int(entry["shadow"]), bounces=int(entry["bounces"]), ambient=v3(entry["ambient"]),
                eye=v3(entry["eye"]), look_at=v3(entry["look_at"]), fov=x(entry["fov"]))


def scenes():
    """{name: S} of the fixture scenes, in the table's order"""
    return {e["name"]: scene_of(e) for e in scene_table()["scenes"]}


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a fixture"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/raytracer_scenes/<name>_WxH.npz: frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    w, h = scene_table()["size"]
    return np.load(os.path.join(GOLDEN, "raytracer_scenes", "%s_%dx%d.npz" % (name, w, h)))


def check_conditions(table, frames, masks):
    """The conditions under which the fixtures say something, over {name: frame} and {name: masks of that frame}: asserted by the
    tool that records them and again of the committed files.  Conditions, not measurements."""
    by_name = {e["name"]: e for e in table["scenes"]}
    assert len(by_name) >= 4
    for name, m in masks.items():
        assert int((m["first_kind"] == 2).sum()) >= 100, (name, "first hits on a sphere", int((m["first_kind"] == 2).sum()))
        assert int((m["first_kind"] == 1).sum()) >= 100, (name, "first hits on a plane", int((m["first_kind"] == 1).sum()))
        assert nan_pixels(frames[name]) == 0, (name, "NaN pixels", nan_pixels(frames[name]))
    assert max(int((m["first_kind"] == 0).sum()) for m in masks.values()) >= 20, "no frame with 20 background pixels"
    assert max(int(m["shadowed"].sum()) for m in masks.values()) >= 30, "no frame with 30 shadowed pixels"
    assert max(int((m["depth"] >= 2).sum()) for m in masks.values()) >= 100, "no frame with 100 second bounces"
    four = [n for n, e in by_name.items() if e["bounces"] == 4]
    assert four and max(int((masks[n]["depth"] >= 3).sum()) for n in four) >= 20, "no 4-bounce frame with 20 third bounces"
    dirs = [n for n, e in by_name.items() if e["light_type"] == LIGHT_DIR]
    assert dirs and max(int(masks[n]["lit"].sum()) for n in dirs) >= 100, "no LIGHT_DIR frame with 100 lit hits"
    assert any(e["lighting"] == 1 for e in by_name.values()) and any(e["shadow"] == 0 for e in by_name.values())
    assert any((len(e["planes"]), len(e["spheres"])) != (6, 3) for e in by_name.values())


# ---- seeded random scenes (tests/test_gpu_raytracer_scene.py, tools/time_raytracer_scene.py) ---------------------------------------------
COUNTS = (0, 1, 2, 7, 16)


def tame_scene(seed, counts=None):
    """all numbers finite, radii in [.1, 2], the camera outside every sphere; counts from COUNTS^2"""
    rng = np.random.default_rng(1000 + seed)
    u = lambda lo, hi, n=None: np.asarray(rng.uniform(lo, hi, size=n), dtype=F)[()]  # noqa: E731
    np_, ns = counts or (int(rng.choice(COUNTS)), int(rng.choice(COUNTS)))
    eye = (u(-1.5, 1.5), u(1, 3), u(6, 8))
    spheres = []
    while len(spheres) < ns:
        o, r = tuple(u(-3, 3, 3) * np.array([1, .5, 1], dtype=F) + np.array([0, 1.5, 0], dtype=F)), u(.1, 2)
        if np.sqrt(sum((float(o[k]) - float(eye[k])) ** 2 for k in range(3))) > float(r) + .25:
            spheres.append((o, r, int(rng.integers(0, 8))))
    walls = [((0, -1, 0), 0.0), ((0, 0, -1), -4.0), ((1, 0, 0), 4.0), ((-1, 0, 0), -4.0), ((0, 1, 0), 6.0)]
    planes = []
    for i in range(np_):
        n, d = walls[i % len(walls)]
        n = tuple(F(c) * u(.5, 2) + u(-.2, .2) for c in n)                   # unnormalised, tilted
        planes.append((n, F(d) + u(-.5, .5) - F(i // len(walls)), int(rng.integers(0, 8))))
    base = u(0, 1, (8, 3))
    return dict(planes=planes, spheres=spheres, base=base, rough=u(.05, 1, 8), ior=u(1, 2, 8),
                refl=np.where(rng.uniform(size=8) < .4, u(.1, 1, 8), F(0)).astype(F),
                light=tuple(u(-3, 3, 3) + np.array([0, 4, 0], dtype=F)), light_type=1 + seed % 2, lighting=(seed // 2) % 2,
                shadow=int(seed % 5 != 0), bounces=1 + seed % 8, ambient=tuple(u(0, .05, 3)), eye=eye, look_at=(u(-.5, .5), u(.5, 1.5), u(-.5, .5)),
                fov=u(.4, 1))
