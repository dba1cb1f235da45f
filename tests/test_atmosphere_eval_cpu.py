"""CPU checks of sbx_atmosphere_eval's references and surface: tests/atmosphere_eval_model.py against the oracle's two hooks on every
ray of the families A-D at every u_time the GPU tests use (bit for bit, NaN == NaN, none left out), the families themselves, and the
declaration / export of the entry point."""
import os
import re

import numpy as np
import pytest

from tests import atmosphere_eval_model as M
from tests.atmosphere_ground_model import sun_dir
from tests.model_common import F, oracle, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hook(name, rays, t):
    o = oracle()
    return np.stack([o.kat(name, [1, 1, 0, 0, t, *r], 3) for r in rays])


@pytest.mark.parametrize("t", M.TIMES)
def test_model_equals_the_oracle_hooks(t):
    rays = M.families()
    assert len(rays) >= 110
    got = M.get_incident_light(rays, sun_dir(t))
    want = hook("atmosphere.get_incident_light", rays, t)
    bad = np.flatnonzero(~same_bits(got, want).all(axis=-1))
    assert bad.size == 0, ("get_incident_light", t, bad[:5], got[bad[:3]], want[bad[:3]])
    got = M.get_sun_light(rays)
    want = hook("atmosphere.get_sun_light", rays, t)
    bad = np.flatnonzero(~same_bits(got, want).all(axis=-1))
    assert bad.size == 0, ("get_sun_light", t, bad[:5], got[bad[:3]], want[bad[:3]])


def test_families_hold_what_they_are_for():
    a, b, c, d = M.family_a(), M.family_b(), M.family_c(), M.family_d()
    assert (len(a), len(b), len(c)) == (40, 40, 20) and len(d) >= 10
    assert np.array_equal(M.families().view(np.uint32), M.families().view(np.uint32))      # deterministic
    assert 10 <= int((a[:, 4] < 0).sum()) <= 30                          # about half of A looks down
    rb = np.linalg.norm(b[:, :3].astype(np.float64), axis=1)
    assert (rb >= 6360e3 - 1).all() and (rb <= 6420e3 + 1).all()
    rc = np.linalg.norm(c[:, :3].astype(np.float64), axis=1)
    assert (rc >= 6.5e6 - 8).all() and (rc <= 4e7 + 8).all()
    assert np.isnan(d).any() and np.isinf(d).any() and (d[:, 3:] == 0).all(axis=1).any()
    # the class (csrc/sbx_atmosphere.h): most of A and B, nothing from space, none of the non-finite or non-unit rays
    q = M.in_class(M.families())
    assert q[:80].sum() >= 64 and not q[80:100].any()
    bad = ~np.isfinite(d).all(axis=1) | (np.abs(np.linalg.norm(d[:, 3:].astype(np.float64), axis=1) - 1) > 1e-3)
    assert not q[100:][bad].any()
    # the hit test splits the set, and get_sun_light returns early on part of it
    sl = M.get_sun_light(M.families())
    assert 0 < int((sl[:, 0] == 0).sum()) < len(sl)
    il = M.get_incident_light(M.families(), (0.0, 1.0, 0.0))
    assert (il == 0).all(axis=1).any() and np.isnan(il).any() and (il > 0).all(axis=1).any()


def test_entry_point_is_declared_bound_and_exported():
    import shaderbox_amd
    from shaderbox_amd import build
    hdr = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"int sbx_atmosphere_eval\(sbx_ctx\* ctx, const char\* fn, const float\* rays, const float\* sun_dir, float\* out,\s*"
                     r"size_t n, void\* stream\);", hdr)
    assert "#define SBX_ABI_VERSION 2" in hdr
    assert "sbx_debug_atmosphere_eval" not in hdr                      # the hook lives in sbx_test.h
    assert "sbx_debug_atmosphere_eval(" in open(os.path.join(ROOT, "include", "sbx_test.h")).read()
    build.build(verbose=False)
    lib = shaderbox_amd.load_library()
    assert len(lib.sbx_atmosphere_eval.argtypes) == 7 and len(lib.sbx_debug_atmosphere_eval.argtypes) == 8
    assert callable(shaderbox_amd.Renderer.atmosphere_eval) and callable(shaderbox_amd.Renderer.atmosphere_eval_counted)
    # without a context every call is refused before it looks at anything else
    assert lib.sbx_atmosphere_eval(None, b"get_incident_light", None, None, None, 0, None) == -1
