"""GPU tests of SBX_APP_CLOUDS_HEIGHT and SBX_APP_CLOUDS_LUMINANCE (src/app_clouds.h with the `#if 0` of illuminate_volume at :97 /
:118 on; include/sbx.h): every layer bit for bit, NaN == NaN, all four channels, against the frames and points the
edited reference header rendered (tests/golden/clouds_builds/) and against tests/clouds_builds_model.py.  Small frames only."""
import os

import numpy as np
import pytest

from oracle import aux_sets
from tests import clouds_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["height", "luminance"]
W, H, T = 96, 54, 1.5

model_frame = frame_cache(lambda build, w, h, t: M.frame(build, w, h, t))


def aux_of(name, **over):
    """the aux set `name` of tests/golden/reference_aux_sets.json (None: the defaults), with `over` on top, as the block the C API takes"""
    import shaderbox_amd
    fields = dict({} if name is None else aux_sets.load()["clouds"][name], **over)
    return shaderbox_amd.AuxClouds.from_buffer_copy(aux_sets.block("clouds", fields).tobytes())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build, variant):
    """what src/app_clouds.h itself rendered with the one line edited: default aux at three times, steer (general sun, 40 / 9 steps),
    yz, degenerate (1 step, no light step) and zero (no step); the default kernels and the plain per-lane one"""
    import torch
    fx = M.fixture(build)
    try:
        renderer.set_variant(variant)
        for name, t, aux_set, want in fx["frames"]:
            aux = None if aux_set is None else aux_of(aux_set)
            assert_same(renderer.render(M.APP_OF[build], W, H, t, aux=aux), want, (build, name, "variant", variant))
        u = fx["points_uniforms"]
        got = renderer.render_points(M.APP_OF[build], int(u[0]), int(u[1]), float(u[4]), torch.from_numpy(fx["points"]))
        assert_same(got, fx["points_out"], (build, "points", "variant", variant))
    finally:
        renderer.set_variant(0)


@pytest.mark.parametrize("build", BUILDS)
def test_odd_frame_equals_the_model(renderer, build):
    """97 is no multiple of the 32 x 2 wave tile, and the horizon cut falls inside waves"""
    assert_same(renderer.render(M.APP_OF[build], 97, 55, T), model_frame(build, 97, 55, T), (build, 97, 55))


# (aux set, fields on top, width, height): a z-only sun, a y-z sun, a general one, sigma on both sides of exp_small_'s threshold, no
# regular frame (|sigma dt| > 80), and a march of more steps than a y table of the ring has rows (the one big table)
VARIANT_CASES = [(None, {}, 256, 144), ("yz", {}, 256, 144), ("steer", {}, 256, 144), ("exp_on", {}, 256, 144), ("exp_off", {}, 256, 144),
                 ("exp_off", {"sun_dir": (0.0, 0.6, -0.8)}, 256, 144), ("steer", {"sigma_scattering": 30.0}, 256, 144),
                 ("long", {"cld_march_steps": 4200}, 64, 36)]
# the kernel each case is meant to reach, (YTAB, REG, LM, SM, GT) of k_clouds as the launch's record names it (sbx_debug_clouds_last_selection;
# GT 3: the hash-table kernels), for the HEIGHT build (no light march: LM 1 whatever the sun) and for the LUMINANCE build
VARIANT_KERNELS = [((1, 1, 1, 1, 3), (1, 1, 1, 1, 3)), ((1, 1, 1, 1, 3), (1, 1, 2, 1, 3)), ((1, 1, 1, 0, 3), (1, 1, 0, 0, 0)),
                   ((1, 1, 1, 1, 3), (1, 1, 1, 1, 3)), ((1, 1, 1, 0, 3), (1, 1, 1, 0, 3)), ((1, 1, 1, 0, 3), (1, 1, 2, 0, 3)),
                   ((1, 0, 1, 0, 0), (1, 0, 0, 0, 0)), ((1, 1, 1, 1, 3), (1, 1, 1, 1, 3))]


def kernel_of(rec):
    return (rec["ytab_used"], rec["reg"], rec["lm"], rec["sm"], rec["gt"])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", range(len(VARIANT_CASES)))
def test_plain_and_default_kernels_agree(renderer, build, case):
    name, over, w, h = VARIANT_CASES[case]
    rng = np.random.default_rng(100 + case)
    t = float(np.float32(rng.uniform(0, 40)))
    aux = aux_of(name, **over)
    try:
        renderer.set_variant(1)
        want = renderer.render(M.APP_OF[build], w, h, t, aux=aux).cpu().numpy()
    finally:
        renderer.set_variant(0)
    assert renderer.clouds_last_selection()["perlane"] == 1
    assert_same(renderer.render(M.APP_OF[build], w, h, t, aux=aux), want, (build, name, over))
    rec = renderer.clouds_last_selection()
    assert rec["perlane"] == 0 and rec["build"] == BUILDS.index(build) + 1 and kernel_of(rec) == VARIANT_KERNELS[case][BUILDS.index(build)], rec
    assert rec["ytab"] == (2 if name == "long" else 1)                   # the one big table / a slot of the ring
    other = renderer.render("clouds", w, h, t, aux=aux).cpu().numpy()
    assert not M.same_bits(other, want).all()                            # and the build is not the shipped one


@pytest.mark.parametrize("build", BUILDS)
def test_captured_launch(renderer, build):
    """a launch recorded into a graph builds its tables inside the capture (the HEIGHT build's luminances with the y rows)"""
    import torch
    out = torch.zeros((H, W, 4), dtype=torch.float32, device=renderer.tdev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            renderer.render(M.APP_OF[build], W, H, T, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, M.fixture(build)["frames"][1][3], (build, "graph"))


# The table-less kernels (every lane's own y terms; HEIGHT: exp_ in place of the luminance table): what a captured launch of more steps
# than a ring table has rows runs, since the one big table is allocated on demand and so never inside a capture (sbx_ytab.hip).  `long`
# at 4200 steps has dt = 137.5 / 4200, so .94 sigma dt <= .2049 (exp_small_, the SM kernels) up to sigma 6.66 and sigma dt <= 80 (the REG
# kernels) up to sigma 2443: (sun, sigma) below reach SM, REG and the plain form under a z-only and under a general sun.
NOTAB_SUNS = {"z": {}, "general": {"sun_dir": (0.3, 0.2, -0.9)}}
NOTAB_SIGMAS = {"sm": 0.15, "reg": 30.0, "plain": 3000.0}
NOTAB_FORMS = {"sm": (1, 1), "reg": (1, 0), "plain": (0, 0)}            # (REG, SM) of the kernel the sigma is meant to reach


@pytest.mark.parametrize("sigma", list(NOTAB_SIGMAS))
@pytest.mark.parametrize("sun", list(NOTAB_SUNS))
@pytest.mark.parametrize("build", BUILDS)
def test_captured_long_march_runs_the_table_less_kernels(renderer, build, sun, sigma):
    import torch
    w, h, t = 64, 36, 0.37
    aux = aux_of("long", cld_march_steps=4200, sigma_scattering=NOTAB_SIGMAS[sigma], **NOTAB_SUNS[sun])
    try:
        renderer.set_variant(1)
        want = renderer.render(M.APP_OF[build], w, h, t, aux=aux).cpu().numpy()
    finally:
        renderer.set_variant(0)
    out = torch.zeros((h, w, 4), dtype=torch.float32, device=renderer.tdev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            renderer.render(M.APP_OF[build], w, h, t, aux=aux, out=out)
    # the record of the captured launch: no y table, no hash table, the light march of the sun (HEIGHT has none: LM 1), REG / SM by sigma
    rec = renderer.clouds_last_selection()
    lm = 1 if build == "height" or sun == "z" else 0
    assert (rec["perlane"], rec["ytab"]) == (0, 0) and kernel_of(rec) == (0, NOTAB_FORMS[sigma][0], lm, NOTAB_FORMS[sigma][1], 0), rec
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, want, (build, sun, sigma, "table-less"))
    assert_same(renderer.render(M.APP_OF[build], w, h, t, aux=aux), want, (build, sun, sigma, "big table"))   # the same frame, eagerly
    rec = renderer.clouds_last_selection()
    assert (rec["ytab_used"], rec["ytab"], rec["reg"], rec["lm"], rec["sm"]) == (1, 2, NOTAB_FORMS[sigma][0], lm, NOTAB_FORMS[sigma][1]), rec
    assert (rec["gt"] != 0) == (lm == 1 and sigma != "plain")           # the z forms of a regular frame read the hash table as well
    if sigma != "plain":                                                 # (there no light reaches a lit sample: LUMINANCE's 0 is the shipped build's 0)
        other = renderer.render("clouds", w, h, t, aux=aux).cpu().numpy()
        assert not M.same_bits(other, want).all()


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    check_rows_host_rows_ranks_and_splits(renderer, M.APP_OF[build], W, H, T, M.fixture(build)["frames"][1][3], cuts=[13, 14, 40])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    check_loopback_exchanges(renderer, M.APP_OF[build], n, W, H, T)


@pytest.mark.parametrize("build", BUILDS)
def test_span_table_is_app_clouds(renderer, build):
    got = renderer.span_table(M.APP_OF[build], 256, 144, T, 8, 4)
    want = renderer.span_table("clouds", 256, 144, T, 8, 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    f = check_rgba8(renderer, M.APP_OF[build], W, H, T)
    assert_same(f, M.fixture(build)["frames"][1][3], (build, "float frame"))


@pytest.mark.parametrize("build", BUILDS)
def test_multi_render(renderer, build):
    check_multi_render(M.APP_OF[build], W, H, T, lambda: M.fixture(build)["frames"][1][3])


@pytest.mark.parametrize("build", BUILDS)
def test_cpp_dropin(tmp_path, build):
    # -DAPP_CLOUDS beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_CLOUDS", "APP_CLOUDS_" + build.upper()], "APP_CLOUDS_" + build.upper())
    for name, t, aux_set, want in M.fixture(build)["frames"][:3]:
        assert_same(run_dropin(exe, W, H, t, tmp_path), want, ("dropin", build, name))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    fx = M.fixture(build)["frames"]
    assert_same(run_sbx_render(tmp_path, M.APP_OF[build], W, H, T), fx[1][3], ("sbx_render --app", build))
    yz = ["--sun", "0,0.6,-0.8"]
    assert_same(run_sbx_render(tmp_path, M.APP_OF[build], W, H, T, yz), fx[4][3], ("sbx_render --app", build, yz))


def test_app_clouds_keeps_its_golden_on_a_shared_context(renderer):
    """the builds share the context's y-table ring: SBX_APP_CLOUDS between and after renders of the new apps, same uniforms"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "clouds_96x54.npz"))
    for key in ("t0", "t0.37", "t2.5"):
        t = float(key[1:])
        for app in ("clouds_height", "clouds", "clouds_luminance", "clouds", "clouds_height"):
            got = renderer.render(app, W, H, t)
            if app == "clouds":
                assert_same(got, z[key], ("clouds", key))
    for build in BUILDS:                                                 # and a table built for SBX_APP_CLOUDS first
        renderer.render("clouds", W, H, 37.25)
        assert_same(renderer.render(M.APP_OF[build], W, H, 37.25), M.fixture(build)["frames"][2][3], (build, "after clouds"))
