"""The element families of sbx_raytracer_eval's tests: what tests/test_gpu_raytracer_eval.py runs on the device and what
tests/test_raytracer_eval_cpu.py holds the conditions of.  A plain module (pytest does not collect it).

    "frame_mirrors", "frame_dirphong"   the 2304 primary rays of a 64 x 36 frame of a fixture scene (4 bounces and Cook-Torrance; LIGHT_DIR
                                        and Phong); their hits are the inputs of "illuminate" and "shadow"
    "box_full", "box_spheres"           1024 seeded rays and points inside tame_scene(seed) with counts (16, 16) and (0, 7): directions
                                        unnormalised, lengths .2 - 2.5; material ids and mat_to_ignore from MATS
    "axes"                              AXES below: exact tangents, zero components, rays that planes and spheres turn away
    "specials"                          NaN, +-inf, 3e38, 1e-40 and -0 in each coordinate slot; NaN, 1e10 and -1e10 as ids

The two box seeds are Phong scenes on purpose: the family draws material ids outside 0..7, whose zero material (roughness 0) makes
illum_cook_torrance's 1 / 0 * exp(-inf) a NaN, and the frame and box families are the ones that hold no NaN row.  Cook-Torrance over
out-of-range ids is in "axes"."""
import numpy as np

from tests import raytracer_eval_model as E
from tests import raytracer_scene_model as M
from tests.model_common import F

SIZE = (64, 36)
MATS = (-3, 0, 1, 2.9, 7, 8, 100)
BOX_SEEDS = {"box_full": (2, (16, 16)), "box_spheres": (3, (0, 7))}      # (seed, counts): lighting = (seed // 2) % 2 = 1, Phong
FAMILIES = ("frame_mirrors", "frame_dirphong", "box_full", "box_spheres", "axes", "specials")

# one floor plane (y = 0, as the Cornell box's plane 0), one sphere, a point light straight above the origin; Cook-Torrance, 3 bounces
_base = np.zeros((8, 3), dtype=F)
_base[0], _base[1], _base[2] = (1, 1, 1), (.7, .7, .7), (.9, .6, .5)
AXES = dict(planes=[((F(0), F(-1), F(0)), F(0), 1)], spheres=[((F(1.5), F(1), F(0)), F(1), 2)], base=_base,
            rough=np.array([0, .5, .25, 0, 0, 0, 0, 0], dtype=F), ior=np.array([1, 1, 1.5, 0, 0, 0, 0, 0], dtype=F),
            refl=np.array([0, 0, 1, 0, 0, 0, 0, 0], dtype=F), light=(F(0), F(4), F(0)), light_type=1, lighting=0, shadow=1, bounces=3,
            ambient=(F(.01), F(.01), F(.01)), eye=(F(0), F(2), F(5)), look_at=(F(0), F(1), F(0)), fov=F(.6))
# origin, direction: the comment names what the row is there for
AXES_RAYS = [
    [0, 3, 2, 0, -1, 0],        # straight down onto the floor at x = the light's x: shadow_line.x is 0, the normalisation records
    [0, 3, -1, 0, -.5, 0],      # the same, an unnormalised direction
    [0, 3, 0, 0, -1, 0],        # the hit is straight under the light: two zero components
    [2.5, 3, 0, 0, -1, 0],      # tangent to the sphere: d2 == radius2, the root is of 0
    [.5, 3, 0, 0, -1, 0],       # tangent on the other side
    [1.5, 2, 2, 0, -2, 0],      # d2 == radius2 by the code's own test under a direction of length 2 (d2 = |rc|^2 - tca^2 = 5 - 4)
    [0, 1, 0, 1, 0, 0],         # parallel to the plane (denom = -0 < 1e-6), hits the sphere head on
    [0, 1, 3, 1, 0, 0],         # parallel to the plane, misses everything
    [0, 1, 3, 0, 1, 0],         # facing away from the plane, a miss
    [1.5, 1, 0, 0, 1, 0],       # from the sphere's centre, upwards
    [1.5, 1, 0, 0, -1, 0],      # from the sphere's centre, down
    [1.5, 1, 0, 1, 1, 1],       # from the sphere's centre, a diagonal
    [1.5, 1, 0, 0, 0, 0],       # from the sphere's centre, a zero direction
    [0, 2, 2, 0, 0, 0],         # a zero direction outside the sphere
    [1.5, 4, 0, 0, -1, 0],      # straight down the sphere's axis: the normal is (0, 1, 0), the mirror ray goes straight up
    [-2, 2, 1, 1, -1, -.25],    # a plain ray onto the sphere
    [-1, 2, 1, .5, -1, .25],    # a plain ray onto the floor
]


def scene_of(name):
    if name.startswith("frame_"):
        return M.scenes()[name[len("frame_"):]]
    if name in BOX_SEEDS:
        seed, counts = BOX_SEEDS[name]
        return M.tame_scene(seed, counts)
    return AXES if name == "axes" else M.scenes()["tilted"]


def _hits(S, rays, mats=None):
    """the hits of rays[n, 6] as "illuminate" inputs [n, 10]: eye = the ray's origin, hit.origin, hit.normal, the material id (mats: ids
    in its place)"""
    h = E.evaluate("raytrace_iteration", S, np.concatenate([rays, np.full((len(rays), 1), -1, dtype=F)], axis=1))
    return np.concatenate([rays[:, :3], h[:, 2:5], h[:, 5:8], (h[:, 1] if mats is None else np.asarray(mats, dtype=F))[:, None]], axis=1).astype(F)


def _of_width(S, rays, win, ignore, mats=None):
    """rays[n, 6] as a family's inputs of width win: with mat_to_ignore; as the hits' shading inputs; as the hits' origins; as they are"""
    if win == 7:
        return np.concatenate([rays, np.asarray(ignore, dtype=F)[:, None]], axis=1).astype(F)
    if win == 10:
        return _hits(S, rays, mats)
    if win == 3:
        return np.ascontiguousarray(_hits(S, rays)[:, 3:6])
    return rays


def _specials(win):
    """a sane row (a ray onto the scene / a hit on its floor) with each special value in each coordinate slot, then the odd ids"""
    base = {7: [.5, 2.5, 6, -.1, -.35, -1, -1], 6: [.5, 2.5, 6, -.1, -.35, -1], 3: [.25, .5, 1],
            10: [.5, 2.5, 6, .25, .5, 1, 0, 1, 0, 2]}[win]
    coords = {7: 6, 6: 6, 3: 3, 10: 9}[win]
    rows = [list(base)]
    for k in range(coords):
        for v in (np.nan, np.inf, -np.inf, 3e38, 1e-40, -0.):
            rows.append(list(base))
            rows[-1][k] = v
    if win in (7, 10):
        for v in (np.nan, 1e10, -1e10):
            rows.append(list(base))
            rows[-1][-1] = v
    return np.array(rows, dtype=F)


def family(name, win):
    """inputs [n, win] of a family; the scene they are meant for is scene_of(name)"""
    S = scene_of(name)
    if name.startswith("frame_"):
        rays = E.primary_rays(S, *SIZE)
        return _of_width(S, rays, win, np.full(len(rays), -1))
    if name in BOX_SEEDS:
        rng = np.random.default_rng(BOX_SEEDS[name][0])
        n = 1024
        o = rng.uniform(-1, 1, size=(n, 3)) * [3.5, 2.6, 5] + [0, 2.9, 1.5]           # x +-3.5, y .3 .. 5.5, z -3.5 .. 6.5
        d = rng.normal(size=(n, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(.2, 2.5, size=(n, 1))
        ids = rng.choice(np.asarray(MATS + (-1, 3, 5), dtype=F), size=n)
        rays = np.concatenate([o, d], axis=1).astype(F)
        if win == 10:           # seeded eyes, points, unnormalised normals and ids of their own: not only what a trace returns
            x = np.concatenate([rays[:, :3], rng.uniform(-1, 1, size=(n, 3)) * [3.5, 2.6, 3.5] + [0, 2.9, 0], rays[:, 3:],
                                rng.choice(np.asarray(MATS, dtype=F), size=(n, 1))], axis=1).astype(F)
            half = _hits(S, rays[:n // 2])
            x[:n // 2, :9] = half[:, :9]                                               # half of them are real hits, under the drawn ids
            return x
        return _of_width(S, rays, win, ids)
    if name == "axes":
        rays = np.array(AXES_RAYS, dtype=F)
        if win == 10:           # the hits under their own materials, then under ids outside 0..7 (Cook-Torrance's zero material) and 0
            return np.concatenate([_hits(S, rays), _hits(S, rays, np.resize(np.asarray([8, -3, 0, 100, 2.9], dtype=F), len(rays)))], axis=0)
        if win == 7:            # every ray with nothing ignored, then with the sphere's material ignored
            return np.concatenate([_of_width(S, rays, 7, np.full(len(rays), -1)), _of_width(S, rays, 7, np.full(len(rays), 2))], axis=0)
        return _of_width(S, rays, win, None)
    return _specials(win)


def recording_ray():
    """one "render" row of "axes" that records (the tangent) for the test of a known re-run"""
    return np.array(AXES_RAYS[3], dtype=F)
