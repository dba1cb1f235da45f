"""GPU tests of sbx_planet_eval (include/sbx.h): APP_PLANET's terrain, cloud shell and shading over the caller's rays and points, bit
for bit (NaN == NaN) over every element against tests/planet_eval_model.py (which tests/test_planet_eval_cpu.py pins to the oracle and
to the reference header's own close-up frame) for all eight functions over the families A-E at two times, through the entry and
through its counted twin; against the SBX_APP_PLANET and SBX_APP_PLANET_CLOSEUP frames; the default form against the plain one; the
wave counts (A never falls back, D and E and variant 1 never run the guarded forms); wave composition, ragged sizes, bounds and
alignment, a stream capture, the argument checks, and host/sbx_render's --planet-view."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import planet_eval_model as M
from tests.app_checks import assert_same, frame_cache, run_sbx_render
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu


@frame_cache
def reference(fn, t, names="abcde"):
    """the model over the input set of `fn` (computed once per key; t is 0 for the functions that do not read it)"""
    return M.evaluate(fn, M.inputs(fn, names), t)


def times(fn):
    return M.TIMES if fn in M.TIME_FNS else (0.0,)


def ev(r, fn, x, t=0.0):
    return r.planet_eval(fn, to_dev(x), t)


def counted(r, fn, x, t=0.0):
    """(out, (waves with every guarded form on, waves that fell back)): the same launch through include/sbx_test.h sbx_debug_planet_eval"""
    return r.planet_eval_counted(fn, to_dev(x), t)


@pytest.mark.parametrize("fn", M.FNS)
def test_against_the_model(renderer, fn):
    x = M.inputs(fn)
    for t in times(fn):
        want = reference(fn, t)
        assert want.shape == (len(x), M.WIDTHS[fn][1])
        assert differing(ev(renderer, fn, x, t), want) == 0, (fn, t)
        out, counts = counted(renderer, fn, x, t)
        assert differing(out, want) == 0, (fn, t, "counted")
        assert sum(counts) == (len(x) + 63) // 64, (fn, counts)


def test_against_the_apps(renderer):
    """linear_to_srgb of "render" over the primary rays of a 48x27 frame is the SBX_APP_PLANET / SBX_APP_PLANET_CLOSEUP frame"""
    w, h = 48, 27
    for app, eye in (("planet", "shipped"), ("planet_closeup", "closeup")):
        rays = M.primary_rays(w, h, *M.EYES[eye])
        for t in M.TIMES:
            frame = renderer.render(app, w, h, t).cpu().numpy().reshape(w * h, 4)
            lin = ev(renderer, "render", rays, t).cpu().numpy()
            assert_same(frame[:, :3], M.linear_to_srgb(lin[:, :3]), (app, t))
            assert 0 < int((lin[:, 3] > 0).sum()) < w * h


def test_variants_same_bits(renderer, variant_restored):
    """default against sbx_set_variant(1) everywhere; under variant 1 no wave runs the guarded forms"""
    for fn in M.FNS:
        x = M.inputs(fn)
        for t in times(fn):
            want = reference(fn, t)
            renderer.set_variant(1)
            out, counts = counted(renderer, fn, x, t)
            assert counts[0] == 0 and counts[1] == (len(x) + 63) // 64, (fn, t, counts)
            assert differing(out, want) == 0 and differing(ev(renderer, fn, x, t), want) == 0, (fn, t, "variant 1")
            renderer.set_variant(0)
            assert differing(ev(renderer, fn, x, t), out.cpu().numpy()) == 0, (fn, t, "default against variant 1")


def test_counts(renderer):
    for fn in M.GUARDED_FNS:
        for t in times(fn):
            a = M.inputs(fn, "a")
            out, (fast, fell) = counted(renderer, fn, a, t)
            assert fell == 0 and fast == (len(a) + 63) // 64, (fn, t, "A", fast, fell)
            assert differing(out, reference(fn, t, "a")) == 0, (fn, t, "A")
            for names in ("d", "e"):
                x = M.inputs(fn, names)
                out, (fast, fell) = counted(renderer, fn, x, t)
                assert fast == 0 and fell == (len(x) + 63) // 64, (fn, t, names, fast, fell)
                assert differing(out, reference(fn, t, names)) == 0, (fn, t, names)
    # an untame u_time takes the plain form for every wave
    a = M.inputs("render", "a")[:128]
    assert counted(renderer, "render", a, 3e8)[1] == (0, 2) and counted(renderer, "render", a, float("nan"))[1] == (0, 2)


def test_tame_specials_run_the_guarded_forms(renderer):
    """B and C never fall back; the finite, small specials of E (zero directions, the centre looking out, directions of length 2 and
    .5, denormals, zero coordinates) run the guarded forms in one wave with rays of A; the zero direction from the exact centre — a
    ground hit at pos = 0, whose shadow march starts along 0/0 — passes the rays' guard and makes its wave shade in the plain form"""
    for names in ("b", "c"):
        x = M.inputs("render", names)
        for t in M.TIMES:
            out, (fast, fell) = counted(renderer, "render", x, t)
            assert fell == 0 and fast == (len(x) + 63) // 64, (names, t, fast, fell)
            assert differing(out, reference("render", t, names)) == 0, (names, t)
    a, e = M.family("a"), M.family("e")
    assert np.isfinite(e[:13]).all() and (np.abs(e[:13]) <= 4).all()
    tame = np.concatenate([a[600:640], e[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]]], axis=0)
    for fn in ("render", "terrain_march"):
        for t in M.TIMES:
            out, counts = counted(renderer, fn, tame, t)
            assert counts == (1, 0), (fn, t, counts)
            assert differing(out, M.evaluate(fn, tame, t)) == 0, (fn, t)
    centre = np.concatenate([tame, e[1:2]], axis=0)
    for t in M.TIMES:
        want = M.render(centre, t)
        assert np.isnan(want[-1, :3]).all()
        out, counts = counted(renderer, "render", centre, t)
        assert counts == (0, 1), (t, counts)
        assert differing(out, want) == 0, t
        out, counts = counted(renderer, "terrain_march", centre, t)         # (no shading: nothing to fall back for)
        assert counts == (1, 0) and differing(out, M.terrain_march(centre, t)) == 0, (t, counts)
    # points with a zero coordinate take the unpaired differences inside the guarded form
    z = M.inputs("sdf_terrain_normal", "e")[-6:]
    pts = np.concatenate([M.inputs("sdf_terrain_normal", "a")[:40], z], axis=0)
    for fn in ("sdf_terrain_normal", "illuminate"):
        x = pts if fn == "sdf_terrain_normal" else np.concatenate([pts, np.linspace(0, 2, len(pts), dtype=F)[:, None]], axis=1)
        out, counts = counted(renderer, fn, x, .37)
        assert counts == (1, 0) and differing(out, M.evaluate(fn, x, .37)) == 0, (fn, counts)


def test_wave_composition_does_not_matter(renderer):
    """A, D and E interleaved so that every wave holds all three kinds give the bits they give apart"""
    for fn, t in (("render", .37), ("terrain_march", 0.0), ("sdf_terrain_normal", 0.0), ("clouds_density", 0.0), ("illuminate", .37),
                  ("sdf_terrain_map", 0.0)):
        parts = [M.inputs(fn, nm) for nm in "ade"]
        x = np.concatenate(parts, axis=0)
        base = np.concatenate([ev(renderer, fn, p, t).cpu().numpy() for p in parts], axis=0)      # evaluated apart
        assert differing(base, np.concatenate([reference(fn, t, nm) for nm in "ade"], axis=0)) == 0, (fn, t)
        n = len(x)
        kind = np.repeat([0, 1, 2], [len(p) for p in parts])
        keys = np.concatenate([(np.arange(len(p)) + .5) / len(p) for p in parts])
        mixed = np.argsort(keys, kind="stable")
        assert sorted(mixed) == list(range(n))
        for w in range(0, n, 64):
            assert set(kind[mixed[w:w + 64]]) == {0, 1, 2}, (fn, w)
        for order in (np.arange(n)[::-1], mixed):
            got, counts = counted(renderer, fn, x[order], t)
            assert differing(got, base[order]) == 0, (fn, t)
            assert differing(ev(renderer, fn, x[order], t), base[order]) == 0, (fn, t)
        assert counts[0] == 0, (fn, counts)                                                       # (mixed: every wave holds a D or E element)
        for i in (0, 63, 64, len(parts[0]) + 3, n - 40, n - 1):                                   # one element per call
            assert differing(ev(renderer, fn, x[i:i + 1], t), base[i:i + 1]) == 0, (fn, t, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 193])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in 4 bytes off a 16-byte boundary, out 4 bytes off too; the 4-, 3-,
    2- and 1-float output widths"""
    cases = []
    for fn in ("render", "sdf_terrain_normal", "sdf_terrain_map", "clouds_density"):
        pick = np.resize(np.arange(len(M.inputs(fn)))[::-1], n)                # from the specials backwards
        cases.append((fn, M.WIDTHS[fn], M.inputs(fn)[pick], reference(fn, 0.0)[pick]))
    check_ragged(renderer, raw_call(renderer, "planet", lead=(ctypes.c_float(0.0),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture, replayed over other rays in the same buffers; the counted twin refuses the capturing stream"""
    lead = (ctypes.c_float(.37),)
    twin = raw_call(renderer, "planet", lead=lead, counts=(ctypes.c_uint * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "planet", lead=lead), "render"), M.rays(), reference("render", .37), 4,
                         refused_twin=partial(twin, "background"))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    rays = torch.from_numpy(M.family("a")[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 4), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr())
    assert lib.sbx_planet_eval(None, b"render", 0.0, rp, op, 4, s) == -1
    bad_args = [(ctx, None, 0.0, rp, op, 4, s), (ctx, b"render", 0.0, None, op, 4, s), (ctx, b"render", 0.0, rp, None, 4, s),
                (ctx, b"density_func", 0.0, rp, op, 4, s), (ctx, b"", 0.0, rp, op, 4, s), (ctx, b"Render", 0.0, rp, op, 4, s),
                (ctx, b"render", 0.0, rp, op, (1 << 31) + 1, s)]
    check_refusals(renderer, lib.sbx_planet_eval, lambda args: lib.sbx_debug_planet_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s), bad_args, out)
    for fn in M.FNS:
        assert lib.sbx_planet_eval(ctx, fn.encode(), 0.0, None, None, 0, s) == 0       # n == 0 touches nothing
        assert renderer.planet_eval(fn, torch.zeros((0, M.WIDTHS[fn][0]))).shape == (0, M.WIDTHS[fn][1])
    with pytest.raises(SbxError):
        renderer.planet_eval("density_func", rays)
    assert lib.sbx_debug_planet_eval(ctx, b"render", 0.0, rp, op, 4, None, s) == -1    # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    # not a render: the launch counter of sbx_stats stays where it is
    before = renderer.stats()["render_launches"]
    assert differing(renderer.planet_eval("render", rays), M.render(M.family("a")[:4])) == 0
    assert renderer.stats()["render_launches"] == before


def test_planet_view_of_sbx_render(renderer, tmp_path):
    """host/sbx_render --planet-view 48 27 with the shipped camera's numbers writes what the model gives over that camera's primary
    rays (the host's FOV, libm's tan of the binary32 angle rounded, has the bits of the model's for 30 degrees)"""
    w, h, t = 48, 27, .37
    assert F(np.tan(np.float64(F(30.) * F(0.017453292519943295)))).view(np.uint32) == M.PB.fov().view(np.uint32)
    got = run_sbx_render(tmp_path, "planet", w, h, t, flags=("--planet-view", str(w), str(h), "0", "0", "-2.5", "0", "0", "2"))
    assert_same(got.reshape(w * h, 4), reference("render", t, "a"), "planet view")
    got = run_sbx_render(tmp_path, "planet", w, h, t, flags=("--planet-view", str(w), str(h), "0", "0", "-2.5", "0", "0", "2", "--fov", "30"))
    assert_same(got.reshape(w * h, 4), reference("render", t, "a"), "planet view, --fov 30")
