"""GPU sweep of SBX_APP_ATMOSPHERE_AIR's run-time tier (and of sbx_atmosphere_air_eval) over the seeded random TAME airs of
tests/caller_sweeps.py: k_atmosphere_air<VIEW, true> and k_atmosphere_air_eval<FN, true> held to
tests/atmosphere_air_model.py bit for bit (NaN == NaN, no tolerance, no pixel left out) where the fast body's written proofs meet
data no fixture has — an eye off the y axis, a camera whose rays dive into the planet, betas that carry tau across the ballot's 80,
a beta of zero or below (the dead-ray exit off), a sun inside the tolerance that is no unit vector.  The tier counters
(sbx_debug_atmosphere_air_launches) show that every launch under variants 0, 2 and 3 was the run-time tier's, never the literal one
and never the plain kernel, so that no comparison is the plain kernel with itself; the eval entry's count of fast waves is the
number of 64-ray chunks the Python class test passes, which is also what tile_bodies says of the frame those rays came from;
tests/test_caller_sweeps_cpu.py shows that the frames mix the bodies.  Then the edges of the domain, and ten launches of one block.
The sibling of tests/test_gpu_caller_sweeps.py, whose egg and vinyl checks stand as they were.

A seed that fails is a finding about csrc/: its block goes into FINDINGS below, by name, and stays there."""
import numpy as np
import pytest

from tests import atmosphere_air_model as M
from tests import atmosphere_eval_model as E
from tests import caller_sweeps as C
from tests.app_checks import assert_same, bits_differ, check_rgba8, edge_points, frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import differing, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu
APP = "atmosphere_air"
CLASSES = tuple(C.CASES[APP])
SIZE = C.AIR_SIZE                                    # 64x36: whole tiles across, half a tile at the top
RAGGED = (97, 61)                                    # ragged both ways, into a poisoned buffer
DENSE = (333, 187)
POISON = -7.25
POINTS = edge_points(*SIZE)                          # off-centre, outside the frame, huge, inf and NaN
FINITE = np.isfinite(POINTS).all(axis=1)
FNS = ("get_incident_light", "get_sun_light")
UP = lambda v: np.nextafter(F(v), F(np.inf))  # noqa: E731

# blocks at which the sweep once differed from the model or from the plain kernel: {name: block as the model's dict}
FINDINGS = {}

model_frame = frame_cache(lambda cls, seed, w, h: M.frame(C.atmosphere_air(cls, seed), w, h))


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


def launched(r, A, variant, what, call):
    """call() is one launch of block A under `variant`: the tier counters move as M.tier_of says, and a launch of a tame block that
    is not variant 1's took neither the literal tier nor the plain kernel"""
    before = r.atmosphere_air_launches()
    got = call()
    after = r.atmosphere_air_launches()
    tier = M.tier_of(A, variant)
    assert after == (before[0] + 1, before[1] + (tier == M.LITERAL), before[2] + (tier == M.PLAIN)), (what, variant, tier, before, after)
    if variant != 1:
        assert tier == M.RUNTIME and after[1:] == before[1:], (what, variant, "not the run-time tier", before, after)
    return got.cpu().numpy()


def check_block(r, A, what, frames):
    """one tame block under variants 0 - 3: the 64x36 frame and the 97x61 frame (into a poisoned buffer) against the model, the point
    list against the model and across variants 0 and 1, the 8-bit frame, the tier of every launch.  frames: (64x36, 97x61) of the model"""
    import torch
    assert M.tier_of(A) == M.RUNTIME and M.refused(A) is None, what
    a = M.as_aux(A)
    frag = torch.from_numpy(POINTS)
    points = {}
    for variant in (0, 1, 2, 3):
        r.set_variant(variant)
        got = launched(r, A, variant, what, lambda: r.render(APP, *SIZE, 0.0, aux=a))
        assert_same(got, frames[0], (what, "64x36 against the model, variant", variant))
        assert (got[..., 3] == 1).all(), (what, "alpha", variant)
        got = launched(r, A, variant, what, lambda: r.render(APP, *RAGGED, 0.0, aux=a, out=poisoned(r, *RAGGED)))
        assert not (got == F(POISON)).any(), (what, "poison left in the 97x61 frame, variant", variant)
        assert_same(got, frames[1], (what, "97x61 against the model, variant", variant))
        points[variant] = launched(r, A, variant, what, lambda: r.render_points(APP, *SIZE, 0.0, frag, aux=a))
    r.set_variant(0)
    want = M.points(A, *SIZE, POINTS[FINITE])
    for variant in (0, 1, 2, 3):
        assert_same(points[variant][FINITE], want, (what, "points against the model, variant", variant))
        assert_same(points[variant], points[1], (what, "every point, inf and NaN among them, against variant 1; variant", variant))
    assert_same(check_rgba8(r, APP, *SIZE, 0.0, aux=a), frames[0], (what, "the float frame beside the 8-bit one"))


@pytest.mark.parametrize("cls", CLASSES)
def test_frames_and_points_are_the_models(renderer, variant_restored, cls):
    for seed in C.CASES[APP][cls]:
        check_block(renderer, C.atmosphere_air(cls, seed), (cls, seed), (model_frame(cls, seed, *SIZE), model_frame(cls, seed, *RAGGED)))


@pytest.mark.parametrize("cls", CLASSES)
def test_dense_frames_are_the_models(renderer, variant_restored, cls):
    """333x187, the first 4 seeds: against the model and against variant 1"""
    for seed in C.CASES[APP][cls][:4]:
        A = C.atmosphere_air(cls, seed)
        a, got = M.as_aux(A), {}
        for variant in (0, 1):
            renderer.set_variant(variant)
            got[variant] = launched(renderer, A, variant, (cls, seed), lambda: renderer.render(APP, *DENSE, 0.0, aux=a, out=poisoned(renderer, *DENSE)))
        assert not (got[0] == F(POISON)).any(), (cls, seed)
        assert_same(got[0], got[1], (cls, seed, "dense frame against variant 1"))
        assert_same(got[0], model_frame(cls, seed, *DENSE), (cls, seed, "dense frame against the model"))


def test_findings_stay_fixed(renderer, variant_restored):
    for name, A in sorted(FINDINGS.items()):
        check_block(renderer, A, name, (M.frame(A, *SIZE), M.frame(A, *RAGGED)))


# ---- the eval entry -------------------------------------------------------------------------------------------------------------------

def fast_chunks(rays):
    """the 64-ray chunks E.in_class finds all in the class; a ragged last chunk counts if its live rays all pass"""
    q = E.in_class(rays)
    return sum(1 for at in range(0, len(rays), 64) if q[at:at + 64].all())


# E.families() in tests/test_gpu_atmosphere_air_eval.py's order: the class rays of A and B first, so that their first chunk is all class
_ALL = E.families()
_FIRST = E.in_class(_ALL) & (np.arange(len(_ALL)) < 80)
FAMILIES = _ALL[np.concatenate([np.flatnonzero(_FIRST), np.flatnonzero(~_FIRST)])]
assert E.in_class(FAMILIES[:64]).all() and not E.in_class(FAMILIES[64:]).all()


def frame_rays(A):
    """the rays the 64x36 frame's lanes hold, in tile order, 64 per tile (a lane past the top edge: the class ray), then FAMILIES"""
    rays, _ = M.held_rays(A, *SIZE)
    tiles = M.tiles_of(rays, np.array(M.CLASS_RAY, dtype=F))
    return np.ascontiguousarray(np.concatenate([tiles.reshape(-1, 6), FAMILIES], axis=0))


@pytest.mark.parametrize("cls", CLASSES)
def test_eval_entry_is_the_model(renderer, variant_restored, cls):
    """the first 4 seeds, both functions, variants 0 and 1; the count of fast waves is the class test's, chunk by chunk, and over
    the frame's own chunks it is tile_bodies' (a wave the app skips holds 64 class rays here)"""
    for seed in C.CASES[APP][cls][:4]:
        A = C.atmosphere_air(cls, seed)
        assert M.tier_of(A, app=False) == M.RUNTIME
        rays = frame_rays(A)
        bodies = M.tile_bodies(A, *SIZE)
        assert fast_chunks(rays[:64 * bodies.size]) == int((bodies != M.PLAIN_BODY).sum()), (cls, seed, "tile_bodies against the class test")
        chunks = fast_chunks(rays)
        assert chunks == int((bodies != M.PLAIN_BODY).sum()) + 1 and 8 <= chunks < (len(rays) + 63) // 64, (cls, seed, chunks, "and FAMILIES' first chunk")
        for fn in FNS:
            want = (M.get_incident_light if fn == FNS[0] else M.get_sun_light)(A, rays)
            for variant in (0, 1):
                renderer.set_variant(variant)
                out, waves = renderer.atmosphere_air_eval_counted(fn, to_dev(rays), M.as_aux(A))
                assert differing(out, want) == 0, (cls, seed, fn, "variant", variant)
                assert waves == (chunks if variant == 0 else 0), (cls, seed, fn, variant, waves, chunks)
        renderer.set_variant(0)


# ---- the edges of the domain ----------------------------------------------------------------------------------------------------------

def _last_true(ok, lo, hi):
    """the largest binary32 in [lo, hi] at which ok holds; ok(lo), not ok(hi), ok monotone between"""
    lo, hi = int(F(lo).view(np.uint32)), int(F(hi).view(np.uint32))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(np.uint32(mid).view(F)) else (lo, mid)
    return np.uint32(lo).view(F)


SUN_EDGE = _last_true(lambda v: M.sun_ok((0., v, 0.)), 1., 1.001)     # the Python rule picks it: |v v - 1| <= 1e-4 in binary32
R_ATM = F(6420e3)
# name: ((block on the bound, its tier), (block a binary32 beyond, its tier)); sun_power 19 keeps the first off the literal tier
EDGES = {
    "sun_dir": ((M.air(.37, sun_dir=(0., SUN_EDGE, 0.), sun_power=19.), M.RUNTIME), (M.air(.37, sun_dir=(0., UP(SUN_EDGE), 0.), sun_power=19.), M.PLAIN)),
    "hR": ((M.air(.37, hR=7994., sun_power=19.), M.RUNTIME), (M.air(.37, hR=UP(7994.), sun_power=19.), M.PLAIN)),
    "eye": ((M.air(.37, eye=(0., R_ATM, 0.)), M.RUNTIME), (M.air(.37, eye=(0., UP(R_ATM), 0.)), M.RUNTIME)),
}


def test_the_edges_are_where_the_rules_put_them():
    assert 1. < float(SUN_EDGE) < 1.0001 and M.sun_ok((0., SUN_EDGE, 0.)) and not M.sun_ok((0., UP(SUN_EDGE), 0.))
    for name, sides in EDGES.items():
        for A, tier in sides:
            assert M.tier_of(A) == tier and M.refused(A) is None, name
            assert C.atmosphere_air_tame(A) == (tier == M.RUNTIME), name


def own_rays(A):
    """the rays of the 64x36 frame's marching pixels alone, in row order"""
    rays, march = M.held_rays(A, *SIZE)
    return np.ascontiguousarray(rays[march])


@pytest.mark.parametrize("name", sorted(EDGES))
def test_the_edge(renderer, variant_restored, name):
    """one value on the bound and the next binary32 beyond it: the frame is the model's on both sides, and the record shows the side.
    The eye's bound is the class's oo <= R^2, judged ray by ray on the device: the tier stays, and beyond it no wave of that eye's
    own rays runs the fast body"""
    for A, tier in EDGES[name]:
        want = M.frame(A, *RAGGED)
        for variant in (0, 3):
            renderer.set_variant(variant)
            before = renderer.atmosphere_air_launches()
            got = renderer.render(APP, *RAGGED, 0.0, aux=M.as_aux(A), out=poisoned(renderer, *RAGGED)).cpu().numpy()
            assert renderer.atmosphere_air_launches() == (before[0] + 1, before[1], before[2] + (tier == M.PLAIN)), (name, tier, variant)
            assert not (got == F(POISON)).any()
            assert_same(got, want, (name, tier, variant))
            assert (got[..., 3] == 1).all()
        renderer.set_variant(0)
        rays = own_rays(A)
        chunks = fast_chunks(rays) if tier == M.RUNTIME else 0
        for fn in FNS:
            out, waves = renderer.atmosphere_air_eval_counted(fn, to_dev(rays), M.as_aux(A))
            assert differing(out, (M.get_incident_light if fn == FNS[0] else M.get_sun_light)(A, rays)) == 0, (name, tier, fn)
            assert waves == chunks, (name, tier, fn, waves, chunks)
    on, beyond = own_rays(EDGES["eye"][0][0]), own_rays(EDGES["eye"][1][0])
    assert fast_chunks(on) >= 8 and not E.in_class(beyond).any(), "the eye on the sphere is of the class, the next one is not"


# ---- sustained launches ---------------------------------------------------------------------------------------------------------------

def test_ten_launches_of_one_block_keep_their_bits(renderer):
    """500x515, ragged tiles, into poisoned buffers: the dispatch-order table over this kernel (a tile a table lost would stay
    poison); ten launches, all of the run-time tier"""
    import torch
    w, h = 500, 515
    A = C.atmosphere_air("ground", 0)
    a = M.as_aux(A)
    before = renderer.atmosphere_air_launches()
    first = None
    for k in range(10):
        got = renderer.render(APP, w, h, 0.0, aux=a, out=poisoned(renderer, w, h))
        torch.cuda.synchronize()
        if first is None:
            first = got.clone()
            assert not bool((first == POISON).any())
        assert bits_differ(got, first) == 0, ("launch", k + 1)
    assert renderer.atmosphere_air_launches() == (before[0] + 10, before[1], before[2])
