"""GPU tests of APP_CLOUDS' lattice-hash table (csrc/kern_clouds.hip GTab / CL_GTAB, csrc/sbx_ytab.hip clouds_hash_table; DESIGN.md
§5.1): the kernels that read their hashes from the context's table render the frames of the per-lane kernel (sbx_set_variant 1: every
lane hashes its own corners, no table of any kind), and the launches that must not touch a table do not.  Every frame goes into a
buffer poisoned with a NaN no kernel computes, every comparison is bit for bit with NaN == NaN, and sbx_debug_clouds_hashtab's
`last_launch_used_table` is asserted wherever a table is expected.  Small frames only."""
import os

import numpy as np
import pytest

from oracle import aux_sets
from tests import clouds_builds_model as M
from tests.app_checks import assert_same
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)
from tests.model_common import F, get_primary_ray, point_cam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.37
GUARD, MIN_RANGE = 512, 1 << 18                       # csrc/sbx_device.h CLOUDS_HASHTAB_GUARD / _MIN_RANGE
SUNS = {"z": None, "yz": (0.0, 0.6, -0.8)}            # the z-only light march (LM == 1) and the y-z one (LM == 2)
APPS = ["clouds", "clouds_height", "clouds_luminance"]   # the three builds that share k_clouds
POISON = 0x7fc0beef


def aux_of(sun):
    import shaderbox_amd
    if sun is None:
        return None
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", {"sun_dir": sun}).tobytes())


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.int32, device=r.tdev).view(torch.float32)


def launch(r, app, w, h, t, **kw):
    """one launch into a poisoned buffer, finished -> the frame as a numpy array (no poison left)"""
    import torch
    out = r.render(app, w, h, t, out=poisoned(r, w, h), **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got.view(np.uint32) == POISON).any(), (app, w, h, t, "pixels left unwritten")
    return got


def perlane(r, app, w, h, t, **kw):
    try:
        r.set_variant(1)
        return launch(r, app, w, h, t, **kw)
    finally:
        r.set_variant(0)


def used_table(r):
    """sbx_debug_clouds_hashtab's `last_launch_used_table`, which is `gt != 0` of the launch's record"""
    used = r.clouds_hashtab()[3]
    assert used == (1 if r.clouds_last_selection()["gt"] else 0)
    return used


def kernel_of(rec):
    """(YTAB, REG, LM, SM, GT) of the k_clouds instantiation the record names"""
    assert rec["perlane"] == 0
    return (rec["ytab_used"], rec["reg"], rec["lm"], rec["sm"], rec["gt"])


@pytest.fixture
def fresh():
    """a context of its own: no table built yet"""
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


# ---- 1. the table's contents -------------------------------------------------------------------------------------------------------
def test_table_holds_the_hash_of_every_index(fresh):
    import torch
    launch(fresh, "clouds", 33, 3, T)
    entries, bias, built, used = fresh.clouds_hashtab()
    assert (built, used) == (1, 1)
    assert bias == MIN_RANGE + GUARD and entries == 2 * MIN_RANGE + 272 + 2 * GUARD
    table = fresh.clouds_hashtab_read(0, entries)
    rng = np.random.default_rng(20)
    idx = np.concatenate([rng.integers(0, entries, 4096), [0, entries - 1, GUARD, entries - 1 - GUARD, bias, bias + 271]])
    arg = (idx - bias).astype(np.float32)              # exact: |i - bias| < 2^24
    want = fresh.math("hash", torch.from_numpy(arg)).cpu().numpy()
    assert np.array_equal(table[idx].view(np.uint32), want.view(np.uint32))


# ---- 2. small frames ---------------------------------------------------------------------------------------------------------------
def test_golden_frame_through_the_table(renderer):
    z = np.load(os.path.join(ROOT, "tests", "golden", "clouds_96x54.npz"))
    got = launch(renderer, "clouds", 96, 54, T)
    assert used_table(renderer) == 1
    assert_same(got, z["t0.37"], "golden clouds_96x54 t0.37")
    assert_same(got, perlane(renderer, "clouds", 96, 54, T), "per-lane")
    assert used_table(renderer) == 0                   # the per-lane kernel reads no table


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("shape", [(96, 54), (33, 3), (520, 501)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("app", APPS)
def test_small_and_ragged_frames_equal_the_per_lane_kernel(renderer, app, shape, sun):
    w, h = shape
    aux = aux_of(SUNS[sun])
    got = launch(renderer, app, w, h, T, aux=aux)
    assert used_table(renderer) == 1, (app, shape, sun)
    assert_same(got, perlane(renderer, app, w, h, T, aux=aux), (app, shape, sun))


# ---- 3. waves that mix marching lanes and lanes given the straight-up ray ---------------------------------------------------------------
def mixed_waves(w, h, mouse):
    """wave tiles (32 x 2 pixels) of the frame in which some lanes march and some do not (the horizon cut dir.y < .05 inside the tile)"""
    fx = np.broadcast_to((np.arange(w, dtype=F) + F(.5))[None, :], (h, w)).ravel()
    fy = np.broadcast_to((np.arange(h, dtype=F) + F(.5))[:, None], (h, w)).ravel()
    pcx, pcy = point_cam(w, h, fx, fy, M.FOV)
    eye, look_at = M.setup_camera(mouse)
    d = get_primary_ray(pcx, pcy, eye, look_at)
    m = (~(d[1] < F(0.05))).reshape(h // 2, 2, w // 32, 32)
    any_, all_ = m.any(axis=(1, 3)), m.all(axis=(1, 3))
    return int((any_ & ~all_).sum())


@pytest.mark.parametrize("sun", list(SUNS))
@pytest.mark.parametrize("h", [52, 56])
def test_horizon_waves(renderer, h, sun):
    """the horizon cut (dir.y < .05, just above the middle of the frame) falls inside a row of wave tiles at these heights: every wave
    of that tile row has marching lanes and lanes on the straight-up ray"""
    w, mouse = 256, (300.0, 0.0)
    assert mixed_waves(w, h, mouse) >= w // 32
    aux = aux_of(SUNS[sun])
    got = launch(renderer, "clouds", w, h, T, mouse=mouse, aux=aux)
    assert used_table(renderer) == 1
    assert_same(got, perlane(renderer, "clouds", w, h, T, mouse=mouse, aux=aux), ("horizon", h, sun))


# ---- 4. growth -----------------------------------------------------------------------------------------------------------------------
def test_a_larger_frame_gets_a_larger_table_and_the_old_one_stays(fresh):
    w, h = 96, 54
    want = {t: perlane(fresh, "clouds", w, h, t) for t in (T, 200.0)}
    assert fresh.clouds_hashtab()[2] == 0
    for k, (t, built) in enumerate([(T, 1), (200.0, 2), (T, 2)]):
        got = launch(fresh, "clouds", w, h, t)
        entries, bias, n, used = fresh.clouds_hashtab()
        assert (n, used) == (built, 1), (k, t)
        assert bias == (MIN_RANGE << (n - 1)) + GUARD
        assert_same(got, want[t], ("growth", k, t))


# ---- 5. launches that must not touch a table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [3000.0, float("inf")], ids=["beyond_the_cap", "non_finite_wind"])
def test_frames_outside_the_table_keep_the_cache_kernels(fresh, t):
    w, h = 96, 54
    got = launch(fresh, "clouds", w, h, t)
    assert fresh.clouds_hashtab() == (0, 0, 0, 0)
    # the cache kernel it keeps: y table (a ring slot), REG, the z-only light march; a wind that is not finite is outside sin_b40_'s
    # domain as well, so no SM there
    rec = fresh.clouds_last_selection()
    assert kernel_of(rec) == (1, 1, 1, 1 if t == 3000.0 else 0, 0) and (rec["ytab"], rec["need_range"], rec["table_range"]) == (1, 0, 0), rec
    assert_same(got, perlane(fresh, "clouds", w, h, t), ("fallback", t))


def test_general_sun_and_point_lists_keep_the_cache_kernels(fresh):
    import torch
    launch(fresh, "clouds", 96, 54, T, aux=aux_of((0.3, 0.2, -0.9)))
    assert fresh.clouds_hashtab()[2:] == (0, 0)
    rec = fresh.clouds_last_selection()
    assert kernel_of(rec) == (1, 1, 0, 1, 0) and (rec["light"], rec["need_range"]) == (0, 0), rec      # the general light march, LDS cache
    pts = torch.tensor([[10.5, 40.5], [3.25, 50.0]], dtype=torch.float32, device=fresh.tdev)
    fresh.render_points("clouds", 96, 54, T, pts)
    torch.cuda.synchronize()
    assert fresh.clouds_hashtab()[2:] == (0, 0)
    rec = fresh.clouds_last_selection()
    assert kernel_of(rec) == (1, 1, 1, 1, 0) and (rec["light"], rec["need_range"], rec["launches"]) == (1, 0, 2), rec   # the z-only march, LDS cache


def test_captured_launch_without_a_table_builds_none(fresh):
    import torch
    w, h = 96, 54
    want = perlane(fresh, "clouds", w, h, T)
    out = poisoned(fresh, w, h)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fresh.render("clouds", w, h, T, out=out)
    assert fresh.clouds_hashtab()[2:] == (0, 0)         # nothing allocated inside the capture: the cache kernel was recorded
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, want, "captured, no table")
    assert_same(launch(fresh, "clouds", w, h, T), want, "eager, after the capture")
    assert fresh.clouds_hashtab()[2:] == (1, 1)


# ---- 6. built on one stream, read on another -------------------------------------------------------------------------------------------
def test_two_streams_without_host_synchronisation(fresh):
    import torch
    w, h = 520, 501
    want = perlane(fresh, "clouds", w, h, T)
    a, b = poisoned(fresh, w, h), poisoned(fresh, w, h)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        fresh.render("clouds", w, h, T, out=a)             # builds the table on sa
    first = fresh.clouds_hashtab()[2:]
    with torch.cuda.stream(sb):
        fresh.render("clouds", w, h, T, out=b)             # reads it on sb
    second = fresh.clouds_hashtab()[2:]
    torch.cuda.synchronize()
    assert first == (1, 1) and second == (1, 1)
    assert_same(a, want, "building stream")
    assert_same(b, want, "reading stream")
    assert_same(launch(fresh, "clouds", w, h, T), want, "single stream")


# ---- 7. with the dispatch order ----------------------------------------------------------------------------------------------------------
def test_frames_under_the_dispatch_order(fresh):
    w, h = 520, 501
    frames = []
    for k in range(5):
        if k == 4:
            assert fresh.tile_order("clouds")[0] >= 1      # the fifth launch runs under a tile-order table
        frames.append(launch(fresh, "clouds", w, h, T))
        assert used_table(fresh) == 1, k
    assert_same(frames[4], frames[0], "fifth frame against the first")
    assert_same(frames[0], perlane(fresh, "clouds", w, h, T), "per-lane")
