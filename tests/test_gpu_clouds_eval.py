"""GPU tests of sbx_clouds_eval (include/sbx.h): APP_CLOUDS' volume and sky over the caller's rays, bit for bit (NaN == NaN) against
tests/clouds_eval_model.py (which tests/test_clouds_eval_cpu.py pins to the oracle) for all five functions over the families A-E,
the four aux sets and both times, through the entry and through its counted twin; against the SBX_APP_CLOUDS frame; the default
form (hashes from the context's table, asserted through the counts) against the plain one; wave composition, ragged sizes, bounds and
alignment, a stream capture, the argument checks, and host/sbx_render's panorama."""
import ctypes
from functools import partial
import ctypes.util

import numpy as np
import pytest

from tests import clouds_eval_model as M
from tests.app_checks import assert_same, frame_cache, run_sbx_render
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu

RAY_FNS = ("render", "render_clouds")                                   # the two that read u_time


@frame_cache
def reference(fn, aux, t):
    """the model over the whole input set of `fn` (computed once per key; t is 0 for the functions that do not read it)"""
    return M.evaluate(fn, M.inputs(fn), t, M.AUX[aux])


def cases():
    return [(fn, aux, t) for fn in M.FNS for aux in M.AUX for t in (M.TIMES if fn in RAY_FNS else (0.0,))]


def ev(r, fn, x, t=0.0, aux="default"):
    return r.clouds_eval(fn, to_dev(x), t, M.AUX[aux])


def counted(r, fn, x, t=0.0, aux="default"):
    """(out, (cells from the table, cells hashed in place)): the same launch through include/sbx_test.h sbx_debug_clouds_eval"""
    return r.clouds_eval_counted(fn, to_dev(x), t, M.AUX[aux])


@pytest.mark.parametrize("aux", list(M.AUX))
def test_against_the_model(renderer, aux):
    for fn, a, t in cases():
        if a != aux:
            continue
        x, want = M.inputs(fn), reference(fn, aux, t)
        assert want.shape == (len(x), M.WIDTHS[fn][1])
        assert differing(ev(renderer, fn, x, t, aux), want) == 0, (fn, aux, t)
        out, counts = counted(renderer, fn, x, t, aux)
        assert differing(out, want) == 0, (fn, aux, t, "counted")
        assert (sum(counts) > 0) == (fn != "render_sky_color"), (fn, counts)


def test_against_the_app(renderer):
    """linear_to_srgb of "render" over the primary rays of a 64x36 frame is the SBX_APP_CLOUDS frame"""
    w, h = 64, 36
    rays = M.primary_rays(w, h)
    for aux in ("default", "general_sun"):
        block = renderer._clouds_aux(M.AUX[aux])
        for t in M.TIMES:
            frame = renderer.render("clouds", w, h, t, aux=block).cpu().numpy().reshape(w * h, 4)
            lin = ev(renderer, "render", rays, t, aux).cpu().numpy()
            assert_same(frame[:, :3], M.linear_to_srgb(lin[:, :3]), (aux, t))
            assert 0 < int((lin[:, 3] > 0).sum()) < w * h


def test_variants_same_bits(renderer, variant_restored):
    """default against sbx_set_variant(1) everywhere; under variant 1 no cell comes from the table"""
    for fn, aux, t in cases():
        x, want = M.inputs(fn), reference(fn, aux, t)
        renderer.set_variant(1)
        out, counts = counted(renderer, fn, x, t, aux)
        assert counts[0] == 0, (fn, aux, t, counts)
        assert differing(out, want) == 0 and differing(ev(renderer, fn, x, t, aux), want) == 0, (fn, aux, t, "variant 1")
        renderer.set_variant(0)
        assert differing(ev(renderer, fn, x, t, aux), out.cpu().numpy()) == 0, (fn, aux, t, "default against variant 1")


def test_counts(renderer):
    abc, d = M.rays("abc"), M.family("d")
    for fn in ("render", "render_clouds", "illuminate_volume"):
        for t in M.TIMES:
            # (render_clouds marches C's rays under the horizon cut too, along dir / dir.y: out of every table)
            tab, here = counted(renderer, fn, M.rays("ab") if fn == "render_clouds" else abc, t)[1]
            assert here == 0 and tab > 0, (fn, t, tab, here)
            tab, here = counted(renderer, fn, d[20:], t)[1]
            assert tab == 0 and here > 0, (fn, t, "far", tab, here)
            tab, here = counted(renderer, fn, d[:20], t)[1]
            assert tab > 0 and here > 0, (fn, t, "near", tab, here)
    for aux in M.AUX:
        pts = M.points()
        tab, here = counted(renderer, "density_func", pts, 0.0, aux)[1]
        assert tab + here == 4 * len(pts) and tab > 0 and here > 0, (aux, tab, here)
    assert counted(renderer, "render_sky_color", M.inputs("render_sky_color"))[1] == (0, 0)


def test_wave_composition_does_not_matter(renderer):
    rays = M.rays()
    n = len(rays)
    na, nd, ne = len(M.rays("abc")), len(M.family("d")), len(M.family("e"))
    kind = np.repeat([0, 1, 2], [na, nd, ne])
    # the three kinds merged evenly (each at its fraction of the way through its own list): near, far and special rays in every wave
    keys = np.concatenate([(np.arange(m) + .5) / m for m in (na, nd, ne)])
    mixed = np.argsort(keys, kind="stable")
    assert sorted(mixed) == list(range(n))
    for w in range(0, n, 64):
        assert set(kind[mixed[w:w + 64]]) == {0, 1, 2}, w
    for fn, aux, t in [("render", "default", 1.5), ("render_clouds", "general_sun", 0.0), ("illuminate_volume", "exp_outside", 0.0),
                       ("render", "cov_one", 1.5)]:
        base = reference(fn, aux, t)
        for order in (np.arange(n)[::-1], mixed):
            got, _ = counted(renderer, fn, rays[order], t, aux)
            back = np.empty_like(base)
            back[order] = got.cpu().numpy()
            assert differing(back, base) == 0, (fn, aux, t)
            assert differing(ev(renderer, fn, rays[order], t, aux), base[order]) == 0, (fn, aux, t)
        for i in (0, 63, 64, 200, na + 3, na + 25, na + nd, na + nd + 7, n - 1):        # one ray per call
            assert differing(ev(renderer, fn, rays[i:i + 1], t, aux), base[i:i + 1]) == 0, (fn, aux, t, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in and out 4 bytes off their allocation's alignment; the 4-, 3- and
    1-float output widths"""
    cases = []
    for fn in ("render", "render_sky_color", "density_func"):
        pick = np.resize(np.arange(len(M.inputs(fn)))[::-1], n)                # from the specials backwards
        cases.append((fn, M.WIDTHS[fn], M.inputs(fn)[pick], reference(fn, "default", 0.0)[pick]))
    check_ragged(renderer, raw_call(renderer, "clouds", lead=(None, ctypes.c_float(0.0))), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture, replayed over other rays in the same buffers; only the bits are asserted, whichever hash path the capture took;
    the counted twin refuses the capturing stream"""
    lead = (None, ctypes.c_float(1.5))
    twin = raw_call(renderer, "clouds", lead=lead, counts=(ctypes.c_uint64 * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "clouds", lead=lead), "render"), M.rays(), reference("render", "default", 1.5), 4,
                         refused_twin=partial(twin, "density_func"))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    rays = torch.from_numpy(M.family("b")[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 4), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr())
    neg_main, neg_light = renderer._clouds_aux({"cld_march_steps": -1}), renderer._clouds_aux({"illum_march_steps": -3})
    assert lib.sbx_clouds_eval(None, b"render", None, 0.0, rp, op, 4, s) == -1
    bad_args = [(ctx, None, None, 0.0, rp, op, 4, s), (ctx, b"render", None, 0.0, None, op, 4, s), (ctx, b"render", None, 0.0, rp, None, 4, s),
                (ctx, b"get_sun_light", None, 0.0, rp, op, 4, s), (ctx, b"", None, 0.0, rp, op, 4, s), (ctx, b"Render", None, 0.0, rp, op, 4, s),
                (ctx, b"render", None, 0.0, rp, op, (1 << 31) + 1, s), (ctx, b"render", ctypes.byref(neg_main), 0.0, rp, op, 4, s),
                (ctx, b"density_func", ctypes.byref(neg_light), 0.0, rp, op, 4, s)]
    check_refusals(renderer, lib.sbx_clouds_eval, lambda args: lib.sbx_debug_clouds_eval(*args[:-1], (ctypes.c_uint64 * 2)(7, 7), s), bad_args, out)
    for fn in M.FNS:
        assert lib.sbx_clouds_eval(ctx, fn.encode(), None, 0.0, None, None, 0, s) == 0      # n == 0 touches nothing
        assert renderer.clouds_eval(fn, torch.zeros((0, M.WIDTHS[fn][0]))).shape == (0, M.WIDTHS[fn][1])
    with pytest.raises(SbxError):
        renderer.clouds_eval("get_sun_light", rays)
    assert lib.sbx_debug_clouds_eval(ctx, b"render", None, 0.0, rp, op, 4, None, s) == -1   # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    # not a render: the launch counter of sbx_stats stays where it is
    before = renderer.stats()["render_launches"]
    assert differing(renderer.clouds_eval("render", rays), M.render(M.family("b")[:4])) == 0
    assert renderer.stats()["render_launches"] == before


def test_panorama_of_sbx_render(renderer, tmp_path):
    """host/sbx_render --clouds-panorama 32 16 writes what clouds_eval "render" gives over the rays the host documents"""
    w, h, t, eye = 32, 16, 1.5, (10.0, 20.0, -30.0)
    libm = ctypes.CDLL(ctypes.util.find_library("m"))                   # the host's own sin and cos
    for f in (libm.sin, libm.cos):
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    pi = 3.14159265358979323846
    rays = np.zeros((h, w, 6), dtype=F)
    rays[..., :3] = eye
    for y in range(h):
        for x in range(w):
            az, el = 2.0 * pi * (x + .5) / w, .5 * pi * (y + .5) / h
            rays[y, x, 3:] = (libm.cos(el) * libm.sin(az), libm.sin(el), -libm.cos(el) * libm.cos(az))
    assert rays[0, :, 4].max() < .05 < rays[1, :, 4].min() and rays[-1, 0, 4] > .99        # from under the horizon cut to the zenith
    got = run_sbx_render(tmp_path, "clouds", w, h, t, flags=("--clouds-panorama", str(w), str(h), "--eye", "10", "20", "-30", "--coverage", ".6"))
    want = renderer.clouds_eval("render", to_dev(rays.reshape(-1, 6)), t, {"cld_coverage": float(F(.6))}).cpu().numpy()
    assert_same(got.reshape(w * h, 4), want, "panorama")
    assert 0 < int((want[:, 3] > 0).sum()) < w * h
