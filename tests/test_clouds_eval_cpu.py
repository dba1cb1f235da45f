"""CPU checks of sbx_clouds_eval's references and surface: tests/clouds_eval_model.py against the oracle — its frames for `render` over
the primary rays of a 16x9 frame under every aux set, both mouse positions and both times, its hooks for density_func,
render_sky_color and illuminate_volume on every element of the families B-E (bit for bit, NaN == NaN, none left out) — the families
themselves, and the declaration / binding / export of the entry point."""
import os
import re

import numpy as np
import pytest

from oracle import aux_sets
from tests import clouds_eval_model as M
from tests.model_common import F, oracle, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def differing(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero(~same_bits(got, want).reshape(len(got), -1).all(axis=-1))


@pytest.mark.parametrize("aux", list(M.AUX))
def test_model_render_equals_the_oracle_frames(aux):
    from oracle.oracle import APP_IDS
    block = aux_sets.block("clouds", M.AUX[aux])
    for mouse in M.MOUSES:
        rays = M.primary_rays(16, 9, mouse)
        for t in M.TIMES:
            want = oracle().render(APP_IDS["clouds"], 16, 9, t, mouse=mouse, aux=block).reshape(16 * 9, 4)
            got = M.render(rays, t, M.AUX[aux])
            bad = differing(M.linear_to_srgb(got[:, :3]), want[:, :3])
            assert bad.size == 0, (aux, mouse, t, bad[:5])
            assert (want[:, 3] == 1).all()


def test_model_equals_the_oracle_hooks():
    o = oracle()
    pts = M.inputs("density_func", "bcde")
    assert len(pts) >= 250
    want = np.array([o.kat("clouds.density_func", [*p, 0.0], 1)[:1] for p in pts], dtype=F)
    bad = differing(M.density_func(pts), want)
    assert bad.size == 0, ("density_func", bad[:5], pts[bad[:3]])
    dirs = M.inputs("render_sky_color", "bcde")
    want = np.array([o.kat("clouds.render_sky_color", list(d), 3)[:3] for d in dirs], dtype=F)
    bad = differing(M.render_sky_color(dirs), want)
    assert bad.size == 0, ("render_sky_color", bad[:5], dirs[bad[:3]])
    rays = M.inputs("illuminate_volume", "bcde")
    for L in ((0.0, 0.0, -1.0), M.AUX["general_sun"]["sun_dir"]):                   # the caller's L: the hook takes it as an argument
        want = np.array([o.kat("clouds.illuminate_volume", [*r[:3], 0.0, *r[3:], *L], 1)[:1] for r in rays], dtype=F)
        bad = differing(M.illuminate_volume(rays, {"sun_dir": L}), want)
        assert bad.size == 0, ("illuminate_volume", L, bad[:5], rays[bad[:3]])


def test_families_hold_what_they_are_for():
    a, b, c, d, e = (M.family(n) for n in "abcde")
    assert (len(a), len(b), len(c), len(d)) == (288, 40, 20, 40) and len(e) >= 10
    assert np.array_equal(M.family_d().view(np.uint32), d.view(np.uint32)) and np.array_equal(M.family_b().view(np.uint32), b.view(np.uint32))
    assert (b[:, 4] >= F(.1)).all() and (np.abs(b[:, :3]) <= 2000).all()
    assert np.allclose(np.linalg.norm(b[:, 3:].astype(np.float64), axis=1), 1, atol=1e-6)
    # B at the default aux, u_time 1.5: rays that end by the alpha > .999 break, rays that stay translucent, rays through clear air
    # (render_clouds returns alpha * smoothstep(0, .2, dir.y), and the factor is positive on B)
    with np.errstate(all="ignore"):
        cl = M.render_clouds(b, 1.5)
        s = M.CB.smoothstep(F(0), F(.2), b[:, 4]).astype(np.float64)
    assert (s > 0).all()
    alpha = cl[:, 3].astype(np.float64) / s
    kinds = (int((alpha > .999 - 1e-6).sum()), int(((alpha > 0) & (alpha <= .999 - 1e-6)).sum()), int((alpha == 0).sum()))      # (the quotient is off by < 1e-6)
    assert min(kinds) >= 5 and sum(kinds) == 40, kinds
    # the :212 branch splits A
    above = ~(a[:, 4] < F(.05))
    assert int(above[:144].sum()) == 110 and 0 < int(above[144:].sum()) < 144
    ra = M.render(a, 1.5)
    assert (ra[~above, 3] == 0).all() and (ra[above, 3] > 0).any()
    # C: under the cut the sky, alpha 0 and a finite colour; on the cut and its upper neighbour the march runs
    cut = F(.05)
    assert {float(np.nextafter(cut, F(0))), float(np.nextafter(cut, F(1))), float(cut), 0.0} <= set(map(float, c[:, 4]))
    assert np.signbit(c[c[:, 4] == 0, 4]).any() and not np.signbit(c[c[:, 4] == 0, 4]).all() and (c[:, 4] < 0).any()
    rc = M.render(c, 1.5)
    under = c[:, 4] < cut
    assert 10 <= int(under.sum()) < 20 and (rc[under, 3] == 0).all() and np.isfinite(rc[:, :3]).all()
    assert np.array_equal(rc[~under, 3].view(np.uint32), M.render_clouds(c[~under], 1.5)[:, 3].view(np.uint32))
    # D: the near half's octave-0 lattice indices lie within the smallest hash table, most of its octave-3 indices do not; the far
    # half has none within the largest table
    for t in M.TIMES:
        near = np.abs(M.lattice_indices(M.march_points(d[:20], t)))
        assert (near[:, 0] <= 2.0 ** 18).all() and (near[:, 3] > 2.0 ** 18).mean() > .5, (t, near.max(axis=0))
        far = np.abs(M.lattice_indices(M.march_points(d[20:], t)))
        assert (far > 2.0 ** 22).all(), t
    assert (np.abs(d[:20, :3]) <= 2e5).all() and (np.abs(d[20:, :3]) <= 3e8).all() and (np.abs(d[20:, :3]) >= 1e8).all()
    assert np.array_equal(d[:, 3:], b[:, 3:])
    # A-C stay inside the smallest table in every octave
    for t in M.TIMES:
        assert (np.abs(M.lattice_indices(M.march_points(np.concatenate([a[above], b]), t))) < 2.0 ** 17).all()
    # E: NaN, inf, the zero direction, non-unit directions, a subnormal dir.y
    assert np.isnan(e).any() and np.isinf(e).any() and (e[:, 3:] == 0).all(axis=1).any()
    assert (np.abs(np.linalg.norm(e[8:10, 3:].astype(np.float64), axis=1) - 1) > .5).all()
    assert ((e[:, 4] != 0) & (np.abs(e[:, 4]) < np.finfo(F).tiny)).any()
    # the point set reaches +-3e9 and holds what the rays first sample
    p = M.points()
    assert np.nanmax(np.abs(p[np.isfinite(p).all(axis=1)])) > 1e9 and len(p) == 2 * len(M.rays("bcde")) + 24


def test_entry_point_is_declared_bound_and_exported():
    import shaderbox_amd
    from shaderbox_amd import build
    hdr = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"int sbx_clouds_eval\(sbx_ctx\* ctx, const char\* fn, const sbx_aux_clouds\* aux, float u_time, const float\* in, "
                     r"float\* out, size_t n,\s*void\* stream\);", hdr)
    assert "#define SBX_ABI_VERSION 2" in hdr
    assert "sbx_debug_clouds_eval" not in hdr                          # the hook lives in sbx_test.h
    assert "sbx_debug_clouds_eval(" in open(os.path.join(ROOT, "include", "sbx_test.h")).read()
    build.build(verbose=False)
    lib = shaderbox_amd.load_library()
    assert len(lib.sbx_clouds_eval.argtypes) == 8 and len(lib.sbx_debug_clouds_eval.argtypes) == 9
    assert callable(shaderbox_amd.Renderer.clouds_eval) and callable(shaderbox_amd.Renderer.clouds_eval_counted)
    R = shaderbox_amd.Renderer
    assert R.EVAL_WIDTHS["clouds"] == M.WIDTHS and R.CLOUDS_EVAL_WIDTHS is R.EVAL_WIDTHS["clouds"]      # one table, stated once
    # without a context every call is refused before it looks at anything else
    assert lib.sbx_clouds_eval(None, b"render", None, 0.0, None, None, 0, None) == -1
    assert lib.sbx_debug_clouds_eval(None, b"render", None, 0.0, None, None, 0, None, None) == -1
