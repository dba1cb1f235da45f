"""CPU tests of the definition of SBX_APP_SDF_AO_SHADOW and SBX_APP_SDF_AO_NORMALS (include/sbx.h):
tests/sdf_ao_builds_model.py against the oracle (the shipped build, everything the three builds share), against the frames the
reference header rendered with one `#if 0` turned on (tests/golden/sdf_ao_builds/, tools/make_golden_builds.py) and,
for the shadow term alone, against a scalar step-by-step march over the oracle's sdf hook.  The name tables:
tests/test_build_families_cpu.py, which also asks every
family the header-selection cases at the end of this file."""
import numpy as np
import pytest

from tests import sdf_ao_builds_model as M
from tests.app_checks import assert_same, check_mainimage_selects
from tests.build_families import FAMILIES

FAMILY = FAMILIES["sdf_ao"]
W, H = FAMILY["size"]
F = np.float32


def golden(build):
    """[(u_time, frame)] of one fixture; the uniforms are u_res, u_mouse, u_time per frame, in the order of the frames"""
    z = M.fixture(build)                            # (which asserts the file's keys and uniforms to be the table's)
    assert len(z["frames"]) == len(z["uniforms"]) == len(FAMILY["uniforms"]) and "points" not in z
    for f, u in zip(z["frames"], z["uniforms"]):
        assert (u[0], u[1], u[2], u[3]) == (W, H, 0, 0)
        assert f.shape == (H, W, 4) and f.dtype == np.float32
    return [(float(u[4]), f) for f, u in zip(z["frames"], z["uniforms"])]


def hits(build, w, h, t):
    parts = {}
    fx = (np.arange(w, dtype=F) + F(.5))[None, :]
    fy = (np.arange(h, dtype=F) + F(.5))[:, None]
    M.main_image(build, w, h, t, fx, fy, parts=parts)
    return parts


# ---- what the three builds share: the shipped build against the oracle --------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 36), (97, 61), (7, 3), (1, 1), (160, 90)])
def test_default_build_equals_the_oracle(oracle, w, h):
    from oracle.oracle import APP_SDF_AO
    # fog falloff 0: the factor is 0 / 0, a NaN frame; a negative density; a falloff large enough for exp to overflow
    for t, aux in [(0.0, None), (0.37, None), (2.5, (0.3, 0.0)), (4.6, (0.02, 1.5)), (9.25, (-0.2, 0.25)), (-3.1, (0.1, 40.0)), (100.5, None)]:
        got = M.frame("default", w, h, t, aux)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_SDF_AO, w, h, t, aux=M.aux_bytes(aux)), ("default", w, h, t, aux))


def test_default_build_points_equal_the_oracle(oracle):
    from oracle.oracle import APP_SDF_AO
    w, h, t = 1920, 1080, 1.3
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(0, 1, size=(150, 2)) * [w, h], rng.uniform(-3, 4, size=(80, 2)) * [w, h],
                          [[0, 0], [w, h], [-.5, -.5], [1e30, 1e30], [-3e38, 5], [np.inf, 5], [5, -np.inf], [np.nan, 5], [np.nan, np.nan]]]).astype(F)
    want = np.stack([oracle.main_image(APP_SDF_AO, w, h, t, x, y) for x, y in pts])
    assert_same(M.main_image("default", w, h, t, pts[:, 0], pts[:, 1]), want, "points")


def test_sdf_normal_and_ao_equal_the_oracles_hooks(oracle):
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.uniform(-4, 4, size=(1500, 3)) * [1.5, 1, 1], rng.uniform(-30, 30, size=(300, 3)),
                        hits("default", 64, 36, 2.5)["p"][::5],
                        [[0, 0, 0], [0, 1, 0], [-1.625, 2.15, 0], [1.625, 2.15, 0], [np.nan, 1, 1], [np.inf, 1, 1], [1e30, -1e30, 3]]]).astype(F)
    u = [64, 36, 0, 0, 0.37]
    d, m = M.sdf(p[:, 0], p[:, 1], p[:, 2])
    want = np.stack([oracle.kat("sdf_ao.sdf", u + list(q), 2) for q in p])
    assert_same(np.stack([d, m], axis=1), want, "sdf")
    assert set(np.unique(m)) == {0, 1, 2, 3, 4, 5}                      # every member of the union wins somewhere
    q = p[:400]
    n = M.sdf_normal((q[:, 0], q[:, 1], q[:, 2]))
    assert_same(np.stack(n, axis=1), np.stack([oracle.kat("sdf_ao.sdf_normal", u + list(x), 3) for x in q]), "sdf_normal")
    ao = M.sdf_ao((q[:, 0], q[:, 1], q[:, 2]), n)
    want = np.stack([oracle.kat("sdf_ao.sdf_ao", u + [n[0][i], n[1][i], n[2][i]] + list(q[i]), 3) for i in range(len(q))])
    assert_same(np.stack([ao, ao, ao], axis=1), want, "sdf_ao")


# ---- the two other builds against the reference header's own frames ------------------------------------------------------------

@pytest.mark.parametrize("build", ["shadow", "normals"])
def test_builds_equal_the_reference_frames(build):
    for t, want in golden(build):
        assert_same(M.frame(build, W, H, t), want, (build, t))


def scalar_shadow(oracle, o, trace):
    """sdf_shadow (src/app_sdf_ao.h:183-207) for one ray, a statement per line, over the oracle's sdf"""
    d_ = M.sun_dir()
    t, umbra = F(0), F(1)
    with np.errstate(all="ignore"):
        for _ in range(20):
            p = [o[k] + d_[k] * t for k in range(3)]
            d = oracle.kat("sdf_ao.sdf", [64, 36, 0, 0, 0] + p, 2)[0]
            if t > F(20.):
                trace.append(1)
                return umbra
            if d < F(.005):
                trace.append(2)
                return F(.05)
            t = t + d
            x = F(32.) * d / t
            umbra = x if x < umbra else umbra                            # min(umbra, x) of the spec: (b < a) ? b : a
    trace.append(0)
    return umbra


def test_shadow_term_equals_a_scalar_march(oracle):
    sd = M.sun_dir()
    pts = []
    for t in (0.37, 2.5, 4.6):
        pr = hits("shadow", 64, 36, t)
        pts.append(pr["p"][pr["hit"]][::13])
    pts.append(np.array([[0, 30, 0], [7, 25, -3], [0, 0.004, 6]], dtype=F))      # the first two leave through `t > end`
    p = np.concatenate(pts).astype(F)
    assert len(p) > 300
    o = tuple(p[:, k] + sd[k] * F(0.05) for k in range(3))              # :271
    tr = {}
    got = M.sdf_shadow(*o, trace=tr)
    how, want = [], []
    for i in range(len(p)):
        want.append(scalar_shadow(oracle, [o[0][i], o[1][i], o[2][i]], how))
    assert_same(got, np.array(want, dtype=F), "sh")
    assert np.array_equal(tr["exit"], np.array(how, dtype=np.int8))
    assert set(how) == {0, 1, 2}                                        # ran out of steps, left through t > end, hit an occluder
    assert tr["exit"][len(p) - 3] == 1 and tr["exit"][len(p) - 2] == 1
    umbra, lit = got == F(.05), got == F(1)
    assert umbra.sum() > 20 and lit.sum() > 20 and (~umbra & ~lit & (got > 0) & (got < 1)).sum() > 20, "umbra, lit and penumbra"


def test_shadow_frames_differ_from_the_shipped_build():
    """The share of hit pixels whose colour the shadow changes, per golden frame: 68 of 1654 (4.1 %) at u_time 0.37, 310 of 1653
    (18.8 %) at 2.5, 146 of 1653 (8.8 %) at 4.6; no pixel that misses the scene changes.  The normals view changes every hit pixel."""
    for build in ("shadow", "normals"):
        for t, g in golden(build):
            hit = hits("default", 64, 36, t)["hit"].reshape(36, 64)
            differ = ~M.same_bits(g, M.frame("default", 64, 36, t)).all(axis=2)
            assert not (differ & ~hit).any(), (build, t)
            share = (differ & hit).sum() / hit.sum()
            print(build, t, int((differ & hit).sum()), int(hit.sum()), share)
            assert share > 0, (build, t, share)


# ---- the app include/sbx_mainimage.hpp selects (every family's, from the table: tests/test_build_families_cpu.py) --------------------

@pytest.mark.parametrize("defines,want", [(["APP_SDF_AO_SHADOW"], "SBX_APP_SDF_AO_SHADOW"), (["APP_SDF_AO_NORMALS"], "SBX_APP_SDF_AO_NORMALS"),
                                          (["APP_SDF_AO", "APP_SDF_AO_SHADOW"], "SBX_APP_SDF_AO_SHADOW"),
                                          (["APP_SDF_AO_NORMALS", "APP_SDF_AO"], "SBX_APP_SDF_AO_NORMALS"), (["APP_SDF_AO"], "SBX_APP_SDF_AO")])
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)
