"""CPU tests of tests/caller_sweeps.py: the conditions under which the sweeps of tests/test_gpu_caller_sweeps.py and
tests/test_gpu_caller_sweeps_air.py say something, asserted of the three models alone (tests/egg_pose_model.py,
tests/vinyl_deck_model.py, tests/atmosphere_air_model.py) over all 12 seeds of all 12 classes.  The generators are deterministic and
every block is tame by the Python statement of the library's rule; and the frames show what the classes are about — legs and egg in
view, discs that are hit and not mostly NaN, steep tilts, every material; airs whose 64x36 frames are lit and whose 8x8 tiles (the
waves of k_atmosphere_air) mix the fast and the plain body, both sides of the tau ballot and the dead-ray exit's cases — so that a
sweep cannot pass by showing nothing.  Conditions, not measurements: a range of a generator is adjusted until they hold, never a
threshold here."""
import numpy as np
import pytest

from tests import atmosphere_air_model as M
from tests import atmosphere_eval_model as E_AIR
from tests import caller_sweeps as C
from tests import egg_pose_model as E
from tests import vinyl_deck_model as D
from tests.app_checks import frame_cache

EGG_SIZE, VINYL_SIZE, AIR_SIZE = (128, 72), (64, 36), C.AIR_SIZE
EGG_CLASSES, VINYL_CLASSES, AIR_CLASSES = tuple(C.CASES["egg_pose"]), tuple(C.CASES["vinyl_deck"]), tuple(C.CASES["atmosphere_air"])

egg_shares = frame_cache(lambda cls, seed: E.shares(E.scene_of(C.egg_pose(cls, seed)), *EGG_SIZE))
vinyl_shares = frame_cache(lambda cls, seed: D.shares(D.scene_of(C.vinyl_deck(cls, seed)), *VINYL_SIZE))


@frame_cache
def air_facts(cls, seed):
    """what the 64x36 frame of an air block shows the run-time tier, from the model alone: counts of tiles (waves) and of pixels"""
    A = C.atmosphere_air(cls, seed)
    w, h = AIR_SIZE
    rays, march = M.held_rays(A, w, h)
    bodies = M.tile_bodies(A, w, h)
    flat = rays.reshape(-1, 6)
    seen = {}
    M._incident_light(A, tuple(flat[:, k] for k in range(3)), tuple(flat[:, 3 + k] for k in range(3)), witness=seen)
    tile = lambda a: M.tiles_of(a.reshape(h, w), False)  # noqa: E731
    valid, marching = tile(np.ones(h * w, dtype=bool)), tile(march)
    in_class = E_AIR.in_class(flat) & march.ravel()
    fast = bodies == M.FAST
    inf, n_march = (tile(seen["od_inf"]) & marching).sum(axis=-1), marching.sum(axis=-1)
    frame = M.frame(A, w, h)
    zero = [k for k in range(3) if A["betaR"][k] == 0 or A["betaM"][k] == 0]
    with np.errstate(all="ignore"):
        shown = sum(int((frame[..., k] > 0).sum()) for k in zero)
    return dict(view=A["view"], lit=C.air_lit_share(A), fast=int(fast.sum()), plain=int((bodies == M.PLAIN_BODY).sum()),
                skipped=int((bodies == M.SKIPPED).sum()), plain_marching=int(((bodies == M.PLAIN_BODY) & (n_march > 0)).sum()),
                fast_marchless=int((fast & (valid & ~marching).any(axis=-1)).sum()),
                fast_both_taus=int((fast & (tile(seen["tau_in"]) & marching).any(axis=-1) & (tile(seen["tau_out"]) & marching).any(axis=-1)).sum()),
                fast_all_inf=int((fast & (n_march > 0) & (inf == n_march)).sum()), fast_some_inf=int((fast & (inf > 0) & (inf < n_march)).sum()),
                fast_exit=int((fast & (inf == 64)).sum()), class_inf=int((in_class & seen["od_inf"]).sum()),
                class_under=int((in_class & seen["under"]).sum()), nan_pixels=int(np.isnan(frame).any(axis=-1).sum()), zero_channel=shown)


def test_the_table_of_cases():
    assert EGG_CLASSES == ("studio", "close", "giant", "spun") and VINYL_CLASSES == ("tilted", "orbit", "wild")
    assert AIR_CLASSES == ("ground", "aloft", "thick", "lopsided", "dusk")
    for classes in C.CASES.values():
        for seeds in classes.values():
            assert len(seeds) == len(set(seeds)) == 12


@pytest.mark.parametrize("app,cls", [(app, cls) for app in C.CASES for cls in C.CASES[app]])
def test_deterministic_tame_and_distinct(oracle, app, cls):
    make, block, tame = {"egg_pose": (C.egg_pose, E.block, C.egg_pose_tame), "vinyl_deck": (C.vinyl_deck, D.block, C.vinyl_deck_tame),
                         "atmosphere_air": (C.atmosphere_air, lambda A: M.block(A).view(np.float32), C.atmosphere_air_tame)}[app]
    blocks = []
    for seed in C.CASES[app][cls]:
        b = block(make(cls, seed))
        assert b.dtype == np.float32 and b.size == (16 if app == "egg_pose" else 32)
        assert b.tobytes() == block(make(cls, seed)).tobytes(), (cls, seed, "the same bytes twice")
        assert tame(make(cls, seed)), (cls, seed)
        blocks.append(b.tobytes())
    assert len(set(blocks)) == len(blocks), (cls, "two seeds gave one block")


def test_the_python_rule_refuses_what_the_library_refuses(oracle):
    """the rule is not `True`: the untame blocks of tests/test_gpu_egg_pose.py and tests/test_gpu_vinyl_deck.py, and the edges"""
    feet = ((.3, 1.3, .2), (-.3, 1.1, -.2))
    for kw in (dict(eye=(np.nan, .25, 5.25)), dict(fov=np.inf), dict(turn_deg=np.nan), dict(eye=(0., 3e19, 5.25)), dict(eye=(0., .25, 5.25), look_at=(0., .25, 5.25)),
               dict(eye=(np.nextafter(np.float32(1e4), np.float32(np.inf)), .25, 5.25)), dict(turn_deg=np.nextafter(np.float32(1e10), np.float32(np.inf))),
               dict(eye=(0., 4., 0.), look_at=(0., 0., 0.))):
        assert not C.egg_pose_tame(E.pose(*feet, **kw)), kw
    assert not C.egg_pose_tame(E.POSES["reach"]) and not C.egg_pose_tame(E.pose((0., 0., .2), feet[1]))        # a NaN knee
    for kw in (dict(eye=(1e4, .25, 5.25)), dict(turn_deg=1e10), dict(turn_deg=-1e10)):
        assert C.egg_pose_tame(E.pose(*feet, **kw)), kw
    for name in ("stride", "bones", "inside"):
        assert C.egg_pose_tame(E.POSES[name]), name
    for kw in (dict(sun_dir=(np.nan, .7, -.5)), dict(platter_deg=np.inf), dict(arm_tilt_deg=np.nan), dict(sun_dir=(-1e5, 4e5, -3e5)),
               dict(eye=(0., 5.75, 6.75), look_at=(0., 5.75, 6.75)), dict(sun_dir=(0., np.nextafter(np.float32(1e4), np.float32(np.inf)), 0.)),
               dict(arm_tilt_deg=np.nextafter(np.float32(1e10), np.float32(np.inf)))):
        assert not C.vinyl_deck_tame(D.deck(.37, **kw)), kw
    assert not C.vinyl_deck_tame(D.DECKS["far"])
    for kw in (dict(sun_dir=(0., 1e4, 0.)), dict(platter_deg=1e10), dict(groove_color=(1e30, 0., 0.)), dict(shininess=-3e38), dict(sun_dir=(0., 0., 0.))):
        assert C.vinyl_deck_tame(D.deck(.37, **kw)), kw
    for name in ("scratch", "coloured", "dusk"):
        assert C.vinyl_deck_tame(D.DECKS[name]), name


def _count(cls, what):
    return sum(1 for seed in C.CASES["egg_pose"][cls] if what(egg_shares(cls, seed)[0]))


@pytest.mark.parametrize("cls", ["studio", "close", "spun"])
def test_egg_frames_show_the_legs_and_the_egg(oracle, cls):
    n = len(C.CASES["egg_pose"][cls])
    assert _count(cls, lambda s: s["legs"] >= .005) * 2 >= n, (cls, "legs", [egg_shares(cls, k)[0]["legs"] for k in C.CASES["egg_pose"][cls]])
    assert _count(cls, lambda s: s["egg"] >= .02) * 2 >= n, (cls, "egg")
    for seed in C.CASES["egg_pose"][cls]:
        assert not np.isnan(egg_shares(cls, seed)[1]).any(), (cls, seed)
        assert (egg_shares(cls, seed)[1][..., 3] == 1).all()


def test_giant_legs(oracle):
    seeds = C.CASES["egg_pose"]["giant"]
    assert _count("giant", lambda s: s["legs"] >= .005) * 3 >= len(seeds), [egg_shares("giant", k)[0]["legs"] for k in seeds]
    for seed in seeds:
        P = C.egg_pose("giant", seed)
        assert float(P["femur"]) + float(P["tibia"]) >= 10., (seed, P["femur"], P["tibia"])


def test_spun_turns_are_rotations(oracle):
    for seed in C.CASES["egg_pose"]["spun"]:
        P = C.egg_pose("spun", seed)
        assert 1e3 <= abs(float(P["turn_deg"])) <= 1e9
        m = np.array(E.rotate_around_y(P["turn_deg"]), dtype=np.float64)
        assert np.isfinite(m).all(), (seed, m)
        assert abs(m[0, 0] ** 2 + m[0, 2] ** 2 - 1.) < 1e-6, (seed, "sine and cosine of one angle")


def test_egg_frames_without_ground_and_without_background(oracle):
    every = [egg_shares(cls, seed)[0] for cls in EGG_CLASSES for seed in C.CASES["egg_pose"][cls]]
    assert sum(1 for s in every if s["ground"] == 0) >= 1
    assert sum(1 for s in every if s["background"] == 0) >= 3


@pytest.mark.parametrize("cls", ["tilted", "orbit"])
def test_vinyl_frames_show_the_deck(oracle, cls):
    seeds = C.CASES["vinyl_deck"][cls]
    good, seen = 0, {k: False for k in ("groove", "dead_wax", "label", "shiny", "logo_pixels")}
    for seed in seeds:
        s, f = vinyl_shares(cls, seed)
        hit = int(s["hit"].sum())
        nan = int(np.isnan(f).any(axis=-1).sum())
        good += hit >= .2 * s["hit"].size and nan * 10 <= hit
        for k in seen:
            seen[k] = seen[k] or s[k] > 0
        assert (f[..., 3] == 1).all()
    assert good * 4 >= 3 * len(seeds), (cls, good)
    assert all(seen.values()), (cls, seen)


def test_tilted_has_steep_tilts(oracle):
    decks = [C.vinyl_deck("tilted", seed) for seed in C.CASES["vinyl_deck"]["tilted"]]
    assert sum(1 for d in decks if abs(float(d["platter_tilt_deg"])) > 30) >= 4
    assert sum(1 for d in decks if abs(float(d["arm_tilt_deg"])) > 30) >= 4
    for d in decks:
        assert tuple(d[k] for k in D.CAMERA_FIELDS) == tuple(D.default_deck(0.)[k] for k in D.CAMERA_FIELDS), "the shipped camera"


def test_orbit_moves_the_camera(oracle):
    for cls in ("orbit", "wild"):
        for seed in C.CASES["vinyl_deck"][cls]:
            d = C.vinyl_deck(cls, seed)
            assert d["eye"] != D.default_deck(0.)["eye"] and d["look_at"] != D.default_deck(0.)["look_at"]
            assert float(d["eye"][1]) > .6, (cls, seed, "above the disc")


def test_wild_frames_hit_something(oracle):
    seeds = C.CASES["vinyl_deck"]["wild"]
    assert sum(1 for seed in seeds if vinyl_shares("wild", seed)[0]["hit"].any()) * 2 >= len(seeds)
    for seed in seeds:
        d = C.vinyl_deck("wild", seed)
        assert all(1. <= abs(float(d[k])) <= 1e9 for k in ("platter_deg", "platter_tilt_deg", "arm_tilt_deg"))
        assert 1e-2 <= np.linalg.norm(np.array(d["sun_dir"], dtype=np.float64)) <= 1e4
    every = np.concatenate([D.block(C.vinyl_deck("wild", seed))[16:] for seed in seeds])
    assert (every < 0).any() and (every > 0).any(), "colours and constants of either sign"


# ---- SBX_APP_ATMOSPHERE_AIR: what the blocks show the run-time tier (tests/atmosphere_air_model.py tile_bodies and the march's witness) ----

def _air_count(cls, what):
    return sum(1 for seed in C.CASES["atmosphere_air"][cls] if what(air_facts(cls, seed)))


def _air_views(classes, view):
    return [(cls, seed) for cls in classes for seed in C.CASES["atmosphere_air"][cls] if air_facts(cls, seed)["view"] == view]


def test_the_air_rule_is_the_librarys(oracle):
    """the rule is not `True`, and no block of the sweep is the literal tier's, is refused or has a unit sun"""
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))  # noqa: E731
    for kw in (dict(hR=up(7994.)), dict(hM=1200.0001), dict(earth_radius=up(6360e3)), dict(atmosphere_radius=6420e3 - 1.), dict(num_samples=15),
               dict(num_samples_light=9), dict(sun_dir=(np.nan, 1., 0.)), dict(sun_dir=(0., 1.0001, 0.)), dict(sun_dir=(np.inf, 0., 0.)), dict(sun_dir=(0., 0., 0.))):
        assert not C.atmosphere_air_tame(M.air(.37, **kw)), kw
    for kw in (dict(betaR=(np.nan, -1., 0.)), dict(eye=(np.inf, 0., 0.)), dict(hg_g=7.), dict(sun_dir=(0., -1., 0.)), dict(fov=np.nan), dict(view=1)):
        assert C.atmosphere_air_tame(M.air(.37, **kw)), kw
    for cls in AIR_CLASSES:
        for seed in C.CASES["atmosphere_air"][cls]:
            A = C.atmosphere_air(cls, seed)
            assert M.tier_of(A) == M.RUNTIME and M.tier_of(A, app=False) == M.RUNTIME and M.refused(A) is None, (cls, seed)
            for variant, tier in ((1, M.PLAIN), (2, M.RUNTIME), (3, M.RUNTIME)):
                assert M.tier_of(A, variant) == tier
            D0 = M.default_air(0.)
            assert all(M._same(A[k], D0[k]) for k in ("earth_radius", "atmosphere_radius", "hR", "hM")) and (A["num_samples"], A["num_samples_light"]) == (16, 8)
            s = np.array(A["sun_dir"], dtype=np.float64)
            assert 1e-9 < abs(float(s @ s) - 1.) < 9.2e-5, (cls, seed, "a sun inside the tolerance that is no unit vector")
            eye = np.array(A["eye"], dtype=np.float64)
            assert np.hypot(eye[0], eye[2]) > 1e6 and eye[1] < 6360e3, (cls, seed, "an eye off the y axis, under the plane y = earth_radius")
            assert (A["betaR"], A["betaM"]) != (D0["betaR"], D0["betaM"])
            positive = all(float(b) > 0 for b in A["betaR"] + A["betaM"])
            assert positive == (cls != "lopsided"), (cls, seed, "AtmAir.dead_ok")


@pytest.mark.parametrize("cls", AIR_CLASSES)
def test_air_frames_are_lit_and_mostly_fast(oracle, cls):
    for seed in C.CASES["atmosphere_air"][cls]:
        f = air_facts(cls, seed)
        assert f["lit"] >= C.LIT_SHARE, (cls, seed, "lit", f["lit"])
        assert f["fast"] >= 8, (cls, seed, "fast tiles", f["fast"])
        assert f["fast"] + f["plain"] + f["skipped"] == 8 * 5


@pytest.mark.parametrize("cls,needed", [("ground", 10), ("thick", 10), ("lopsided", 10), ("aloft", 4), ("dusk", 4)])
def test_air_frames_mix_the_bodies(oracle, cls, needed):
    """a wave that marches the plain body beside fast ones, and a fast wave some of whose lanes hold the class ray instead of a march"""
    got = _air_count(cls, lambda f: f["plain_marching"] >= 1 and f["fast_marchless"] >= 1)
    assert got >= needed, (cls, got)


def test_thick_air_crosses_the_tau_ballot_inside_a_fast_wave(oracle):
    for seed in C.CASES["atmosphere_air"]["thick"]:
        assert air_facts("thick", seed)["fast_both_taus"] >= 1, seed
        A = C.atmosphere_air("thick", seed)
        assert max(float(b) for b in A["betaR"]) > 3 * .3 * 22.4e-6 and max(float(b) for b in A["betaM"]) > 3 * .3 * 21e-6


def test_air_rays_that_dive_into_the_planet(oracle):
    """the dead-ray exit's cases.  Every dome block: a fast wave all of whose marching lanes reach an infinite optical depth and one in
    which some do; in every class whose blocks carry the exit, a fast wave whose 64 lanes all do (the exit's own break); view 1 with
    the eye off the axis: class rays that dive"""
    for cls, seed in _air_views(AIR_CLASSES, 0):
        f = air_facts(cls, seed)
        assert f["fast_all_inf"] >= 1 and f["fast_some_inf"] >= 1, (cls, seed, f)
    for cls in ("ground", "aloft", "thick", "dusk"):
        assert _air_count(cls, lambda f: f["fast_exit"] >= 1) >= 1, cls
    cameras = _air_views(("aloft", "dusk"), 1)
    assert sum(1 for cls, seed in cameras if air_facts(cls, seed)["class_inf"] >= 1) >= 4, cameras
    assert len(_air_views(("aloft",), 1)) >= 3 and len(_air_views(("dusk",), 1)) >= 3 and len(_air_views(("aloft", "dusk"), 0)) >= 6


def test_lopsided_air_shows_its_odd_beta(oracle):
    """without the exit a zero beta under an infinite optical depth is 0 * inf: NaN pixels; or the channel whose beta is zero is lit"""
    assert _air_count("lopsided", lambda f: f["nan_pixels"] >= 1 or f["zero_channel"] >= 1) >= 6
    odd = [min(float(b) for b in C.atmosphere_air("lopsided", seed)["betaR"] + C.atmosphere_air("lopsided", seed)["betaM"])
           for seed in C.CASES["atmosphere_air"]["lopsided"]]
    assert any(v < 0 for v in odd) and any(v == 0 for v in odd)


def test_dusk_air_marches_light_into_the_ground(oracle):
    for seed in C.CASES["atmosphere_air"]["dusk"]:
        assert air_facts("dusk", seed)["class_under"] >= 1, seed


def test_the_witness_changes_nothing_and_the_tiles_are_the_kernels(oracle):
    """_incident_light with a witness returns the bits it returns without; tile_bodies at a ragged size: lanes past the edge have no
    vote, and a tile is skipped exactly where none of its pixels marches"""
    A = C.atmosphere_air("aloft", 0)
    rays = M.held_rays(A, 24, 16)[0].reshape(-1, 6)
    seen = {}
    with_witness = M._incident_light(A, tuple(rays[:, k] for k in range(3)), tuple(rays[:, 3 + k] for k in range(3)), witness=seen)
    assert np.array_equal(with_witness.view(np.uint32), M.get_incident_light(A, rays).view(np.uint32))
    assert set(seen) == set(M.WITNESS) and all(v.dtype == bool and v.shape == (len(rays),) for v in seen.values())
    for cls, seed, size in (("ground", 0, (97, 61)), ("aloft", 1, (97, 61)), ("dusk", 3, (64, 36))):
        A = C.atmosphere_air(cls, seed)
        w, h = size
        bodies, (rays, march) = M.tile_bodies(A, w, h), M.held_rays(A, w, h)
        assert bodies.shape == ((h + 7) // 8, (w + 7) // 8)
        ok = E_AIR.in_class(rays.reshape(-1, 6)).reshape(h, w)
        for ty in range(bodies.shape[0]):
            for tx in range(bodies.shape[1]):
                m, c = march[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8], ok[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
                want = M.SKIPPED if not m.any() else M.FAST if c.all() else M.PLAIN_BODY
                assert bodies[ty, tx] == want, (cls, seed, ty, tx)
        assert E_AIR.in_class(np.array([M.CLASS_RAY], dtype=np.float32)).all()
