"""CPU checks of sbx_planet_eval's references and surface: tests/planet_eval_model.py against the oracle — its `planet` frame for
`render` over the shipped camera's primary rays of a 32x18 frame at u_time 0 and .37, its hooks planet.sdf_terrain_map and
planet.sdf_terrain_normal at every point of the point set — and against the 64x36 frame at u_time .37 that the reference's own header
rendered from the close-up eye (tests/golden/planet_builds/), all bit for bit with NaN == NaN and no element left out; terrain_march
against the parts of planet_builds_model.render; the kinds of ray the families must hold, asserted on the model alone; and the
declaration / binding / export of the entry point."""
import os
import re

import numpy as np

from tests import planet_builds_model as PB
from tests import planet_eval_model as M
from tests.model_common import F, oracle, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def differing(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero(~same_bits(got, want).reshape(len(got), -1).all(axis=-1))


def test_model_render_equals_the_oracle_frames():
    from oracle.oracle import APP_IDS
    w, h = 32, 18
    rays = M.primary_rays(w, h, *M.EYES["shipped"])
    for t in M.TIMES:
        want = oracle().render(APP_IDS["planet"], w, h, t).reshape(w * h, 4)
        got = M.render(rays, t)
        bad = differing(M.linear_to_srgb(got[:, :3]), want[:, :3])
        assert bad.size == 0, (t, bad[:5])
        assert 0 < int((got[:, 3] > 0).sum()) < w * h


def test_model_render_equals_the_reference_headers_closeup_frame():
    fx = PB.fixture("closeup")
    w, h, t = (int(fx["uniforms"][0][0]), int(fx["uniforms"][0][1]), float(fx["uniforms"][0][4]))
    assert (w, h) == (64, 36) and t == float(F(.37))
    want = fx["frames"][0].reshape(w * h, 4)
    got = M.render(M.primary_rays(w, h, *M.EYES["closeup"]), t)
    bad = differing(M.linear_to_srgb(got[:, :3]), want[:, :3])
    assert bad.size == 0, bad[:5]
    assert np.isnan(want[:, :3]).any()              # the frame's NaN pixels are compared too


def test_model_equals_the_oracle_hooks():
    o = oracle()
    pts = M.inputs("sdf_terrain_map")
    assert len(pts) >= 300
    want = np.array([o.kat("planet.sdf_terrain_map", list(map(float, p)), 2)[:2] for p in pts], dtype=F)
    bad = differing(M.sdf_terrain_map(pts), want)
    assert bad.size == 0, ("sdf_terrain_map", bad[:5], pts[bad[:3]])
    want = np.array([o.kat("planet.sdf_terrain_normal", list(map(float, p)), 3)[:3] for p in pts], dtype=F)
    bad = differing(M.sdf_terrain_normal(pts), want)
    assert bad.size == 0, ("sdf_terrain_normal", bad[:5], pts[bad[:3]])


def test_terrain_march_agrees_with_the_builds_model():
    w, h, t = 32, 18, .37
    for build, eye in (("default", "shipped"), ("closeup", "closeup")):
        parts = {}
        PB.frame(build, w, h, t, parts=parts)
        tm = M.terrain_march(M.primary_rays(w, h, *M.EYES[eye]), t)
        atm = tm[:, 0] < PB.HIT_T
        assert np.array_equal(atm, parts["atm"]) and np.array_equal(tm[:, 2] < PB.TERR_EPS, parts["ground"]), build
        assert (tm[~atm, 1:] == np.array([0, 1, PB.MAX_HEIGHT], dtype=F)).all()           # the initialisers of :323-324
        assert 0 < int(atm.sum()) < w * h and 0 < int(parts["ground"].sum()) < int(atm.sum())


def test_families_hold_what_they_are_for():
    """Asserted on the model alone: families A-C at u_time .37 hold every kind of ray the GPU test is to compare."""
    a, b, c, d, e = (M.family(n) for n in "abcde")
    assert (len(a), len(b), len(c), len(d)) == (48 * 27, 24 * 14, 96, 64) and len(e) >= 30
    assert len(M.rays()) < 4000
    tr = M.trace(M.rays("abc"), .37)
    atm, ground, alpha, shadow = tr["atm"], tr["ground"], tr["alpha"], tr["shadow"]
    assert int((~atm).sum()) >= 50                                                          # an atmosphere miss
    assert int((atm & ~ground & (alpha > 0)).sum()) >= 20                                   # sky under cloud
    assert int((ground & (shadow == 1)).sum()) >= 50 and int((ground & (shadow == F(.7))).sum()) >= 5
    assert int((atm & ~ground & (tr["t"] > PB.MAX_RAY_DIST)).sum()) >= 20                   # a march that ends by t > max_ray_dist
    r = np.linalg.norm(c[:, :3].astype(np.float64), axis=1)
    ic = len(a) + len(b)
    # origins inside the shell: intersect_sphere gives up where the centre lies behind the ray (tca < 0), so some miss the shell they are in
    assert ((r[:32] > 1.04) & (r[:32] < 1.4)).all() and int(atm[ic:ic + 32].sum()) >= 10 and int((~atm[ic:ic + 32]).sum()) >= 5
    # origins with |o| < 1: t0 < 0 there, hit.origin is the shell's far crossing and the march leaves the planet without a ground hit
    assert (r[64:] < 1).all() and int(atm[ic + 64:].sum()) >= 10 and not ground[ic + 64:].any()
    # D: 10^3, 10^6 and 10^9 away; the 10^3 rays meet the planet
    rd = np.linalg.norm(d[:, :3].astype(np.float64), axis=1)
    assert np.allclose(rd[:40], 1e3, rtol=1e-6) and np.allclose(rd[40:52], 1e6, rtol=1e-6) and np.allclose(rd[52:], 1e9, rtol=1e-6)
    assert int(M.trace(d, .37, clouds=False)["ground"][:40].sum()) >= 20
    # E: NaN and both inf in each slot, a zero direction, the exact centre, denormals, directions of length 2 and .5
    for slot in range(6):
        assert np.isnan(e[:, slot]).any() and (e[:, slot] == np.inf).any() and (e[:, slot] == -np.inf).any()
    assert (e[:, 3:] == 0).all(axis=1).any() and (e[:, :3] == 0).all(axis=1).any()
    assert ((e != 0) & (np.abs(e) < np.finfo(F).tiny)).any()
    n = np.linalg.norm(e[:15, 3:].astype(np.float64), axis=1)
    assert (np.abs(n - 2) < 1e-6).sum() >= 2 and (np.abs(n - .5) < 1e-6).sum() >= 2
    te = M.trace(e, .37)
    assert te["ground"][1] and np.isnan(te["rgb"][1]).all()                                 # the hit at pos = 0
    # the point set: zero coordinates (the unpaired normal path), coordinates of 10^6 and 10^9, NaN
    p = M.points()
    assert (p == 0).any(axis=1).sum() >= 6 and np.isnan(p).any() and np.nanmax(np.abs(p[np.isfinite(p).all(axis=1)])) > 1e8
    for fn in M.FNS:
        assert M.inputs(fn).shape[1] == M.WIDTHS[fn][0]


def test_entry_point_is_declared_bound_and_exported():
    import shaderbox_amd
    from shaderbox_amd import build
    hdr = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"int sbx_planet_eval\(sbx_ctx\* ctx, const char\* fn, float u_time, const float\* in, float\* out, size_t n,\s*"
                     r"void\* stream\);", hdr)
    assert "#define SBX_ABI_VERSION 2" in hdr
    assert "sbx_debug_planet_eval" not in hdr                          # the hook lives in sbx_test.h
    assert "sbx_debug_planet_eval(" in open(os.path.join(ROOT, "include", "sbx_test.h")).read()
    build.build(verbose=False)
    lib = shaderbox_amd.load_library()
    assert len(lib.sbx_planet_eval.argtypes) == 7 and len(lib.sbx_debug_planet_eval.argtypes) == 8
    assert callable(shaderbox_amd.Renderer.planet_eval) and callable(shaderbox_amd.Renderer.planet_eval_counted)
    R = shaderbox_amd.Renderer
    assert R.EVAL_WIDTHS["planet"] == M.WIDTHS and R.PLANET_EVAL_WIDTHS is R.EVAL_WIDTHS["planet"]      # one table, stated once
    # without a context every call is refused before it looks at anything else
    assert lib.sbx_planet_eval(None, b"render", 0.0, None, None, 0, None) == -1
    assert lib.sbx_debug_planet_eval(None, b"render", 0.0, None, None, 0, None, None) == -1
