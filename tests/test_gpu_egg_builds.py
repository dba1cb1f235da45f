"""GPU tests of SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL (src/app_egg.h without its `#define BEZIER` / with its `#if 1` at :46 off;
include/sbx.h): every layer bit for bit, NaN == NaN, all four channels, against tests/egg_builds_model.py — and
against the frames and points the edited reference header rendered (tests/golden/egg_builds/)."""
import numpy as np
import pytest

from tests import egg_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, edge_points, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

BUILDS = ["straight", "oval"]
F = np.float32
TIMES = (0.0037, 0.2, -0.41, 1.3)                                       # at 1.3 the turntable has carried the figure out of view


model_frame = frame_cache(lambda build, w, h, t: M.frame(build, w, h, t, threads=16))


def golden(build):
    z = M.fixture(build)
    return [(float(u[4]), f) for u, f in zip(z["uniforms"], z["frames"])], z["points"], z["points_uniforms"], z["points_out"]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (96, 54), (257, 130), (640, 360)])
def test_frames(renderer, build, w, h):
    for t in TIMES:
        want = model_frame(build, w, h, t)
        assert (want[..., 3] == 1).all()
        assert_same(renderer.render("egg_" + build, w, h, t, mouse=(300.0, 120.0)), want, (build, w, h, t))   # u_mouse does not enter


@pytest.mark.parametrize("build", BUILDS)
def test_frames_1080p(renderer, build):
    w, h, t = 1920, 1080, 0.02
    assert_same(renderer.render("egg_" + build, w, h, t), model_frame(build, w, h, t), (build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build):
    """what src/app_egg.h itself rendered with the one line edited, in every kernel form"""
    import torch
    frames, pts, u, want = golden(build)
    try:
        for variant in (0, 1, 2, 3):
            renderer.set_variant(variant)
            for t, g in frames:
                assert_same(renderer.render("egg_" + build, 96, 54, t), g, (build, t, "variant", variant))
            got = renderer.render_points("egg_" + build, int(u[0]), int(u[1]), float(u[4]), torch.from_numpy(pts))
            assert_same(got, want, (build, "points", "variant", variant))
    finally:
        renderer.set_variant(0)


def test_shipped_build_still_equals_the_oracle(renderer, oracle):
    from oracle.oracle import APP_EGG
    w, h, t = 320, 180, 0.2
    want = oracle.render(APP_EGG, w, h, t)
    assert_same(renderer.render("egg", w, h, t), want, "egg")
    assert_same(model_frame("default", w, h, t), want, "model")
    others = []
    for build in BUILDS:                                                 # and the new apps are other frames
        others.append(renderer.render("egg_" + build, w, h, t).cpu().numpy())
        assert not M.same_bits(others[-1], want).all()
    assert not M.same_bits(others[0], others[1]).all()


@pytest.mark.parametrize("build", BUILDS)
def test_variants_same_bits(renderer, build):
    import torch
    app = "egg_" + build
    w, h, t = 1920, 1080, 0.02
    pts = edge_points(w, h)
    got = {}
    try:
        for v in (0, 1, 2, 3):
            renderer.set_variant(v)
            got[v] = (renderer.render(app, w, h, t).cpu().numpy(), renderer.render_points(app, w, h, t, torch.from_numpy(pts)).cpu().numpy())
    finally:
        renderer.set_variant(0)
    for v in (1, 2, 3):
        assert_same(got[v][0], got[0][0], (build, "frame variant 0 vs", v))
        assert_same(got[v][1], got[0][1], (build, "points variant 0 vs", v))
    assert_same(got[0][0], model_frame(build, w, h, t), (build, "frame vs model"))
    assert_same(got[0][1], M.main_image(build, w, h, t, pts[:, 0], pts[:, 1]), (build, "points vs model"))
    assert_same(renderer.main_image_batch(app, w, h, t, pts[:64]), got[0][1][:64], (build, "batch"))
    for i in [0, 1, 400, 701, 750, 755, len(pts) - 1, len(pts) - 4]:
        c = renderer.main_image(app, w, h, t, (float(pts[i, 0]), float(pts[i, 1])))
        assert_same(np.asarray(c, dtype=np.float32), got[0][1][i], (build, "main_image", i))


def test_main_image_centre_hits_alternate_between_the_builds(renderer):
    """sbx_main_image serves a pixel centre from the frame cached for (app, uniforms): the three builds, asked in turn on one context
    with equal uniforms, each get their own pixel — at pixels where the builds' frames differ"""
    w, h, t = 96, 54, 0.02
    frames = {b: model_frame(b, w, h, t) for b in M.BUILDS}
    pixels = []
    for b in BUILDS:
        ys, xs = np.nonzero(~M.same_bits(frames[b], frames["default"]).all(axis=2))
        assert len(xs) > 0
        pixels += [(int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1]))]
    for _ in range(2):
        for x, y in pixels:
            for b in M.BUILDS:
                c = renderer.main_image(M.APP_OF[b], w, h, t, (x + .5, y + .5))
                assert_same(np.asarray(c, dtype=np.float32), frames[b][y, x], (b, "centre", x, y))


def test_full_frames_alternate_between_the_builds(renderer):
    """a dispatch-order table is keyed by the app: back-to-back launches of one standing scene, the builds taking turns in runs long
    enough for a table to be built and adopted, keep returning each build's own frame"""
    w, h, t = 1920, 1080, 0.02
    first = {}
    for rnd in range(2):
        for b in M.BUILDS:
            for k in range(6):
                got = renderer.render(M.APP_OF[b], w, h, t)
                if b not in first:
                    first[b] = got.clone()
            assert_same(got, first[b].cpu().numpy(), (b, "round", rnd))
            if rnd == 1:                                                    # (round 1's launches had finished when round 2 began: the
                assert renderer.tile_order(M.APP_OF[b])[0] >= 1, b         # table is due behind round 2's first launch at the latest)
    for b in BUILDS:
        assert_same(first[b], model_frame(b, w, h, t), (b, "vs model"))
        assert not M.same_bits(first[b].cpu().numpy(), first["default"].cpu().numpy()).all()


@pytest.mark.parametrize("build", BUILDS)
def test_extreme_times_run_the_plain_kernel(renderer, build):
    """beyond |u_time| = 1e8, and for inf / NaN, the rotations are whatever the spec's reduction returns and the plain kernel runs
    (sbx_capi.hip tame_time): same operations as the model on whatever the matrices are"""
    for t in (3e8, -1e30, float("inf"), float("nan")):
        assert_same(renderer.render("egg_" + build, 64, 36, t), M.frame(build, 64, 36, t), (build, t))


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    w, h, br, t = 640, 360, 8, 0.2
    check_rows_host_rows_ranks_and_splits(renderer, "egg_" + build, w, h, t, model_frame(build, w, h, t), cuts=[13, 14, 300], block_rows=br)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    """the span exchange (whole rows, as APP_EGG) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    w, h, t = 1000, 333, 0.2
    check_loopback_exchanges(renderer, "egg_" + build, n, w, h, t)


@pytest.mark.parametrize("build", BUILDS)
def test_span_table_gives_whole_rows(renderer, build):
    """sbx_span_table has no cost model for the scene: whole rows, as for APP_EGG"""
    w, h, t = 640, 360, 0.2
    table, pix, width = renderer.span_table("egg_" + build, w, h, t, 8, 2)
    ref = renderer.span_table("egg", w, h, t, 8, 2)
    assert (table[:, 0] == 0).all() and (table[:, 1] == w).all() and width == w
    assert np.array_equal(table, ref[0]) and np.array_equal(pix, ref[1]) and width == ref[2]


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    w, h, t = 800, 450, 0.2
    check_rgba8(renderer, "egg_" + build, w, h, t)


def test_precision_tier_is_ignored(renderer):
    w, h, t = 257, 130, 0.2
    try:
        for build in BUILDS:
            renderer.set_precision("exact")
            a = renderer.render("egg_" + build, w, h, t).cpu().numpy()
            renderer.set_precision("1e-4")
            assert_same(renderer.render("egg_" + build, w, h, t), a, (build, "tier"))
    finally:
        renderer.set_precision("exact")


@pytest.mark.parametrize("build", BUILDS)
def test_multi_render(renderer, build):
    w, h, t = 640, 360, 0.2
    check_multi_render("egg_" + build, w, h, t, lambda: model_frame(build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_cpp_dropin(tmp_path, build):
    # -DAPP_EGG beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_EGG", "APP_EGG_" + build.upper()], "APP_EGG_" + build.upper())
    for w, h, t in [(257, 130, 0.2), (96, 54, 0.0037)]:
        assert_same(run_dropin(exe, w, h, t, tmp_path), model_frame(build, w, h, t), ("dropin", build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    w, h = 257, 130
    for t in (0.2, -0.41):
        assert_same(run_sbx_render(tmp_path, "egg_" + build, w, h, t), model_frame(build, w, h, t), ("sbx_render --app egg_" + build, t))
