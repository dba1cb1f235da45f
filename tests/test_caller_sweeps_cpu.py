"""CPU tests of tests/caller_sweeps.py: the conditions under which the sweep of tests/test_gpu_caller_sweeps.py says something, asserted
of the two models alone (tests/egg_pose_model.py, tests/vinyl_deck_model.py) over all 12 seeds of all 7 classes.  The generators are
deterministic and every block is tame by the Python statement of the library's rule; and the frames show what the classes are
about — legs and egg in view, discs that are hit and not mostly NaN, steep tilts, every material — so that a sweep cannot pass by
showing nothing.  Conditions, not measurements: a range of a generator is adjusted until they hold, never a threshold here."""
import numpy as np
import pytest

from tests import caller_sweeps as C
from tests import egg_pose_model as E
from tests import vinyl_deck_model as D
from tests.app_checks import frame_cache

EGG_SIZE, VINYL_SIZE = (128, 72), (64, 36)
EGG_CLASSES, VINYL_CLASSES = tuple(C.CASES["egg_pose"]), tuple(C.CASES["vinyl_deck"])

egg_shares = frame_cache(lambda cls, seed: E.shares(E.scene_of(C.egg_pose(cls, seed)), *EGG_SIZE))
vinyl_shares = frame_cache(lambda cls, seed: D.shares(D.scene_of(C.vinyl_deck(cls, seed)), *VINYL_SIZE))


def test_the_table_of_cases():
    assert EGG_CLASSES == ("studio", "close", "giant", "spun") and VINYL_CLASSES == ("tilted", "orbit", "wild")
    for classes in C.CASES.values():
        for seeds in classes.values():
            assert len(seeds) == len(set(seeds)) == 12


@pytest.mark.parametrize("app,cls", [(app, cls) for app in C.CASES for cls in C.CASES[app]])
def test_deterministic_tame_and_distinct(oracle, app, cls):
    make, block, tame = (C.egg_pose, E.block, C.egg_pose_tame) if app == "egg_pose" else (C.vinyl_deck, D.block, C.vinyl_deck_tame)
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
