"""GPU sweep of SBX_APP_EGG_POSE and SBX_APP_VINYL_DECK (and of sbx_egg_eval / sbx_vinyl_eval) over the seeded random TAME poses and decks
of tests/caller_sweeps.py: the culled, witnessed kernels held to tests/egg_pose_model.py and
tests/vinyl_deck_model.py bit for bit (NaN == NaN, no tolerance, no pixel left out) where the bounds, the hot rectangle and the
hardware min / max are derived from data no fixture has — bent knees, bones of thousands of units, turns of 1e9 degrees, a camera on
any side of the deck, tilts up to 90 degrees, an un-normalised sun.  The launch records (sbx_debug_egg_pose_launches,
sbx_debug_vinyl_deck_launches) show that the host judged every block tame, so that no comparison is the plain kernel with itself;
tests/test_caller_sweeps_cpu.py shows that the frames are not empty.  Then the edge of the tame domain, and ten launches of one block.
(The airs of SBX_APP_ATMOSPHERE_AIR that tests/caller_sweeps.py also generates: tests/test_gpu_caller_sweeps_air.py.)

A seed that fails is a finding about csrc/: its block goes into FINDINGS below, by name, and stays there."""
import numpy as np
import pytest

from tests import caller_sweeps as C
from tests import egg_pose_model as E
from tests import vinyl_deck_model as D
from tests.app_checks import assert_same, bits_differ, edge_points
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F, same_bits

pytestmark = pytest.mark.gpu
MODEL = {"egg_pose": E, "vinyl_deck": D}
MAKE = {"egg_pose": C.egg_pose, "vinyl_deck": C.vinyl_deck}
CLASSES = [(app, cls) for app in MODEL for cls in C.CASES[app]]      # (SBX_APP_ATMOSPHERE_AIR's classes: tests/test_gpu_caller_sweeps_air.py)
SIZE = (128, 72)                                     # the frame compared with the model
DENSE = (333, 187)                                   # legs and tonearm several pixels wide, tiles ragged both ways: device only
EDGE = (67, 35)
POISON = -7.25
_E = edge_points(*SIZE)
POINTS = np.concatenate([_E[:256], _E[-17:]])        # 256 off-centre fragCoords, then the corners, the huge values, inf and NaN
FINITE = np.isfinite(POINTS).all(axis=1)

# blocks at which the sweep once differed from the model or from the plain kernel: {name: (app, block as the model's dict)}
FINDINGS = {}


def launches(r, app):
    return r.egg_pose_launches() if app == "egg_pose" else r.vinyl_deck_launches()


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


def check_block(r, app, block, what):
    """one tame block: the 128x72 frame and the point list against the model and under every variant, the dense frame across variants,
    and the launch record"""
    import torch
    M = MODEL[app]
    a, S = M.as_aux(block), M.scene_of(block)
    frag = torch.from_numpy(POINTS)
    want, want_points = M.frame(S, *SIZE), M.points(S, *SIZE, POINTS[FINITE])
    frames, points, dense = {}, {}, {}
    for variant in (0, 1, 2, 3):
        r.set_variant(variant)
        before = launches(r, app)
        frames[variant] = r.render(app, *SIZE, 0.0, aux=a).cpu().numpy()
        if variant in (0, 1):
            points[variant] = r.render_points(app, *SIZE, 0.0, frag, aux=a).cpu().numpy()
        if variant != 2:
            dense[variant] = r.render(app, *DENSE, 0.0, aux=a, out=poisoned(r, DENSE[0], DENSE[1])).cpu().numpy()
        after = launches(r, app)
        assert after[0] > before[0] and after[1] == before[1], (what, variant, "the host sent a tame block to the reference form", before, after)
    r.set_variant(0)
    assert_same(frames[0], want, (what, "frame against the model"))
    assert (frames[0][..., 3] == 1).all(), (what, "alpha")
    for variant in (1, 2, 3):
        assert_same(frames[variant], frames[0], (what, "frame, variant", variant))
    assert not (dense[0] == F(POISON)).any(), (what, "poison left in the dense frame")
    for variant in (1, 3):
        assert_same(dense[variant], dense[0], (what, "dense frame, variant", variant))
    assert_same(points[0][FINITE], want_points, (what, "points against the model"))
    assert_same(points[0], points[1], (what, "points, variant 1"))


@pytest.mark.parametrize("app,cls", CLASSES)
def test_frames_and_points_are_the_models(renderer, variant_restored, app, cls):
    for seed in C.CASES[app][cls]:
        check_block(renderer, app, MAKE[app](cls, seed), (app, cls, seed))


def test_findings_stay_fixed(renderer, variant_restored):
    for name, (app, block) in sorted(FINDINGS.items()):
        check_block(renderer, app, block, name)


# ---- the eval entries -------------------------------------------------------------------------------------------------------------------

EGG_FNS = {"sdf": 3, "sdf_normal": 3, "shadowmarch": 6, "render_scene": 6}
VINYL_FNS = {"sdf": 3, "sdf_normal": 3, "sdf_shadow": 6, "illuminate": 7, "render": 6}
VINYL_WITNESSED = ("sdf", "sdf_normal", "sdf_shadow", "render")
MATERIALS = [-3, 0, 1, 1, 2, 2, 2.9, 3, 4, 5, 6, 100]           # as tests/test_gpu_vinyl_eval.py draws them


def eval_inputs(app, block, seed):
    """rays [n, 6] and points [n, 3] of a block: the primary rays of its own camera over a 32x18 grid and a point along each, then
    256 points within .2 of the knees and feet (or of the tonearm's pivot) and a ray from each in a random direction; n = 832"""
    rng = np.random.default_rng([31, seed])
    M = MODEL[app]
    fx, fy = (np.arange(32, dtype=F) + F(.5))[None, :], (np.arange(18, dtype=F) + F(.5))[:, None]
    got = M.primary_rays(block, 32, 18, fx, fy)
    ro, rd = got[-2], got[-1]
    n = rd[0].size
    rays = np.stack([np.full(n, ro[0]), np.full(n, ro[1]), np.full(n, ro[2]), rd[0], rd[1], rd[2]], axis=1).astype(F)
    along = (rays[:, :3] + rays[:, 3:] * rng.uniform(0, 9, size=(n, 1)).astype(F)).astype(F)
    if app == "egg_pose":
        S = E.scene_of(block)
        R = C.rot_y(block["turn_deg"])
        joints = np.array([C.world(R, -np.array(S[k], dtype=np.float64)) for k in ("knee_l", "knee_r", "left_foot", "right_foot")])
    else:
        joints = C.PIVOT[None, :]
    near = joints[rng.integers(len(joints), size=256)] + rng.uniform(-.2, .2, size=(256, 3)) / np.sqrt(3.)
    d = rng.normal(size=(256, 3)) * rng.uniform(.2, 2.5, size=(256, 1))
    rays = np.concatenate([rays, np.concatenate([near, d], axis=1).astype(F)], axis=0)
    pts = np.concatenate([along, near.astype(F)], axis=0)
    assert len(rays) == len(pts) <= 4096 and np.isfinite(rays).all() and (np.abs(rays) <= 1e4).all() and (np.abs(pts) <= 1e4).all()
    return rays, pts, rng


def egg_model(fn, S, x):
    with np.errstate(all="ignore"):
        if fn == "sdf":
            return np.stack(E.sdf(S, x[:, 0], x[:, 1], x[:, 2]), axis=1).astype(F)
        if fn == "sdf_normal":
            return E.sdf_normal(S, x[:, 0], x[:, 1], x[:, 2])
        o, d = tuple(x[:, k] for k in range(3)), tuple(x[:, k] for k in range(3, 6))
        if fn == "shadowmarch":
            return E.shadowmarch(S, o, d)[:, None]
        rgb, depth = E.render_scene(S, o, d)
        return np.concatenate([rgb, depth[:, None]], axis=1).astype(F)


def vinyl_model(fn, S, x):
    with np.errstate(all="ignore"):
        a, b = tuple(x[:, k] for k in range(3)), tuple(x[:, k] for k in range(3, 6)) if x.shape[1] >= 6 else None
        if fn == "sdf":
            return np.stack(D.sdf(S, *a), axis=1).astype(F)
        if fn == "sdf_normal":
            return np.stack(D.sdf_normal(S, a), axis=1).astype(F)
        if fn == "sdf_shadow":
            return D.sdf_shadow(S, a, b)[:, None]
        if fn == "illuminate":
            return D.illuminate(S, a, b, D.to_int(x[:, 6]))
        rgb, t, mat = D.render(S, a, b)
        return np.concatenate([rgb, t[:, None], mat[:, None]], axis=1).astype(F)


def differing(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((~same_bits(got, want).reshape(len(want), -1).all(axis=-1)).sum())


@pytest.mark.parametrize("app,cls", CLASSES)
def test_eval_entries_are_the_models(renderer, variant_restored, app, cls):
    """the first 4 seeds of the class: every function against the model under variants 0 and 1; every wave of the launch took the
    culled, witnessed form under variant 0, and under variant 2 (the witness's test edge) waves re-ran"""
    import torch
    M = MODEL[app]
    fns, counted = (EGG_FNS, renderer.egg_eval_counted) if app == "egg_pose" else (VINYL_FNS, renderer.vinyl_eval_counted)
    for seed in C.CASES[app][cls][:4]:
        block = MAKE[app](cls, seed)
        a, S = M.as_aux(block), M.scene_of(block)
        rays, pts, rng = eval_inputs(app, block, seed)
        eye = np.broadcast_to(np.array(block["eye"], dtype=F), pts.shape)
        shading = np.concatenate([eye, pts, rng.choice(np.asarray(MATERIALS, dtype=F), size=(len(pts), 1))], axis=1).astype(F)
        for fn, win in fns.items():
            x = np.ascontiguousarray({3: pts, 6: rays, 7: shading}[win])
            want = (egg_model if app == "egg_pose" else vinyl_model)(fn, S, x)
            waves = (len(x) + 63) // 64
            for variant in (0, 1, 2):
                renderer.set_variant(variant)
                out, counts = counted(fn, torch.from_numpy(x), a)
                assert differing(out, want) == 0, (app, cls, seed, fn, "variant", variant)
                if variant == 0:
                    assert counts[0] + counts[1] == waves and counts[0] > 0, (app, cls, seed, fn, counts, waves)
                elif variant == 1:
                    assert counts == (0, 0), (app, cls, seed, fn, counts)
                elif app == "egg_pose" or fn in VINYL_WITNESSED:
                    assert counts[0] + counts[1] == waves and counts[1] > 0, (app, cls, seed, fn, "variant 2", counts, waves)
            renderer.set_variant(0)


# ---- the edge of the tame domain ----------------------------------------------------------------------------------------------------------

UP = lambda v: np.nextafter(F(v), F(np.inf))  # noqa: E731
_FEET = ((.45, 1.25, .35), (-.3, 1.05, -.1))
EDGES = {
    "egg_pose": {
        "eye.x": lambda v: E.pose(*_FEET, turn_deg=35., eye=(v, 1., 4.5), look_at=(0., 0., 0.), fov=.8),
        "eye.y": lambda v: E.pose(*_FEET, turn_deg=35., eye=(2., v, 4.5), look_at=(0., 0., 0.), fov=.8),
        "turn_deg": lambda v: E.pose(*_FEET, turn_deg=v, eye=(2., 1., 4.5), look_at=(0., 0., 0.), fov=.8),
        "-turn_deg": lambda v: E.pose(*_FEET, turn_deg=-v, eye=(2., 1., 4.5), look_at=(0., 0., 0.), fov=.8),
    },
    "vinyl_deck": {
        "eye.z": lambda v: D.deck(.37, eye=(0., 5.75, v)),
        "platter_deg": lambda v: D.deck(.37, platter_deg=v),
        "-platter_deg": lambda v: D.deck(.37, platter_deg=-v),
        "sun_dir.y": lambda v: D.deck(.37, sun_dir=(-.2, v, -.6)),
        "-sun_dir.x": lambda v: D.deck(.37, sun_dir=(-v, .8, -.6)),
    },
}
EDGE_OF = lambda field: 1e10 if field.endswith("_deg") else 1e4  # noqa: E731


@pytest.mark.parametrize("app,field", [(app, field) for app in EDGES for field in EDGES[app]])
def test_the_tame_edge(renderer, variant_restored, app, field):
    """a value exactly at the bound is tame, the next binary32 above it is not: the record says so, the Python rule says so, and the
    frame is the model's on both sides"""
    M, tame = MODEL[app], (C.egg_pose_tame if app == "egg_pose" else C.vinyl_deck_tame)
    for value, is_tame in ((F(EDGE_OF(field)), True), (UP(EDGE_OF(field)), False)):
        block = EDGES[app][field](value)
        assert tame(block) == is_tame, (field, value)
        want = M.frame(M.scene_of(block), *EDGE)
        for variant in (0, 3):
            renderer.set_variant(variant)
            before = launches(renderer, app)
            got = renderer.render(app, *EDGE, 0.0, aux=M.as_aux(block), out=poisoned(renderer, *EDGE)).cpu().numpy()
            assert launches(renderer, app) == (before[0] + 1, before[1] + (0 if is_tame else 1)), (field, value, variant)
            assert not (got == F(POISON)).any()
            assert_same(got, want, (field, float(value), variant))
            assert (got[..., 3] == 1).all()


# ---- sustained launches ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("app,cls,seed", [("egg_pose", "close", 0), ("vinyl_deck", "orbit", 0)])
def test_ten_launches_of_one_block_keep_their_bits(renderer, app, cls, seed):
    """500x515, ragged tiles, into poisoned buffers: the dispatch-order table over a scene no fixture has (a tile a table lost would
    stay poison)"""
    import torch
    w, h = 500, 515
    a = MODEL[app].as_aux(MAKE[app](cls, seed))
    before = launches(renderer, app)
    first = None
    for k in range(10):
        got = renderer.render(app, w, h, 0.0, aux=a, out=poisoned(renderer, w, h))
        torch.cuda.synchronize()
        if first is None:
            first = got.clone()
            assert not bool((first == POISON).any())
        assert bits_differ(got, first) == 0, ("launch", k + 1)
    assert launches(renderer, app) == (before[0] + 10, before[1])
